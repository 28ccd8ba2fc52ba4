"""mlm_pack_blocks / mlm_unpack_blocks on the CPU: the rule of mlmapping_amd/csrc/mlm_pack.h — argument checks, the code of a cell, the
size of a record, the header, the validator — run as the device phases run it by tests/cpp/pack_driver.cpp, built with g++
-fsanitize=address,undefined, and held byte for byte to the contract in numpy (tests/pack_ref.py).  The decoder is held to the reference
over every single-byte corruption and every truncation of a small stream; the sanitizer shows that nothing beyond `bytes` is read."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pack_ref as ref
from tests.test_fuse_plan import cube_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
NS = [2, 3, 4, 8]
NBLOCKS = [0, 1, 2, 63, 64, 65, 257]
LO_MIN, LO_MAX = np.float32(-2.0), np.float32(3.5)
PLANES = ("keys", "log_odds", "occ", "infl")
DTYPES = {"keys": np.int32, "log_odds": np.float32, "occ": np.uint8, "infl": np.uint8}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pack")
    exe = d / "pack_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pack_driver.cpp"), "-o", str(exe)])

    def call(head, blobs):
        with open(d / "in.bin", "wb") as f:
            f.write(np.array(list(head) + [0] * (24 - len(head)), dtype=np.int64).tobytes())
            for b in blobs:
                f.write(b)
        subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:96], dtype=np.int64)
        return {"status": int(head[0]), "code": int(head[1]), "where": int(head[2]), "summary": head[3:11].copy(), "text": raw[96:192].split(b"\0")[0].decode()}, raw[192:]

    def pack(m, n, flags=0, cap_bytes=None, stream=True, n_arg=None, given=(True, True, True, True), key_lo=None, key_dims=None, misaligned=False,
             lo_min=LO_MIN, lo_max=LO_MAX):
        nb = len(m["keys"])
        if cap_bytes is None:
            cap_bytes = ref.HEADER + nb * (ref.DIR + 16 + 7 * 8 * ref.words(n ** 3) + 4 * n ** 3) + 8
        lo3 = [0, 0, 0] if key_lo is None else list(key_lo)
        d3 = [0, 0, 0] if key_dims is None else list(key_dims)
        head = [0, n, nb if n_arg is None else n_arg, flags, ref.f32_bits(lo_min), ref.f32_bits(lo_max), cap_bytes, int(stream), *[int(g) for g in given],
                int(key_lo is not None), int(key_dims is not None), *lo3, *d3, int(misaligned)]
        rows = nb if given[0] and (n_arg is None or n_arg > 0) else 0
        blobs = [np.ascontiguousarray(m[k][:rows], dtype=DTYPES[k]).tobytes() for k, g in zip(PLANES, given) if g]
        blobs.append(np.ascontiguousarray(m.get("collapsed", np.zeros(nb, np.uint8))[:rows], dtype=np.uint8).tobytes())
        out, rest = call(head, blobs)
        assert len(rest) == cap_bytes
        out["stream"] = rest
        return out

    def unpack(buf, n, cap=None, outputs=15, flags=0, stream=True, misaligned=False, rows_hint=0):
        C = n ** 3
        cap = rows_hint + 1 if cap is None else cap
        out, rest = call([1, n, len(buf), flags, cap, outputs, int(stream), int(misaligned)], [bytes(buf)])
        at, rows = 0, max(cap, 0)
        for k, cols in (("keys", 3), ("log_odds", C), ("occ", C), ("infl", C)):
            size = rows * cols * np.dtype(DTYPES[k]).itemsize
            out[k] = np.frombuffer(rest[at:at + size], dtype=DTYPES[k]).reshape(rows, cols)
            at += size
        assert at == len(rest)
        return out

    return pack, unpack


def wild(rng, keys, C, kinds=None):
    """blocks of every kind the contract names: wild; blank; blank but for one -0.0f; blank but for infl[C-1]; saturated at lo_min / lo_max;
    literals only; a literal only in the last cell; NaN bits"""
    nb = len(keys)
    b = {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": rng.uniform(-3.0, 5.5, size=(nb, C)).astype(np.float32),
         "occ": rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(nb, C)), "infl": rng.choice(np.frombuffer(b"uuo", dtype=np.uint8), size=(nb, C))}
    kind = rng.integers(0, 9, size=nb) if kinds is None else np.asarray(kinds)
    lo, bits = b["log_odds"], b["log_odds"].view(np.uint32)
    for s in range(nb):
        k = int(kind[s])
        if k == 0:  # wild, with clamps and zeros sprinkled in
            pick = rng.integers(0, 4, size=C)
            lo[s][pick == 1], lo[s][pick == 2], lo[s][pick == 3] = LO_MIN, LO_MAX, 0.0
            continue
        if k <= 5 or k == 7:
            lo[s], b["occ"][s], b["infl"][s] = 0.0, ref.U, ref.U
        if k == 2:
            lo[s][rng.integers(C)] = -0.0
        elif k == 3:
            b["infl"][s][C - 1] = ref.O
        elif k == 4:
            lo[s] = np.where(rng.random(C) < 0.5, LO_MIN, LO_MAX)
            b["occ"][s] = np.where(lo[s] == LO_MAX, ref.O, ref.F)
        elif k == 5:  # literals only
            lo[s] = (rng.uniform(0.1, 3.0, size=C)).astype(np.float32)
        elif k == 6:  # NaN bits, an infinity, a subnormal
            bits[s][rng.integers(C)] = 0x7FC00001
            bits[s][rng.integers(C)] = 0xFF800000
            bits[s][rng.integers(C)] = 0x00000001
        elif k == 7:  # a literal only in the last cell
            lo[s][C - 1] = 1.25
    return b


def same_rows(got, m, nb, what):
    for k in PLANES:
        w = np.ascontiguousarray(m[k], dtype=DTYPES[k])
        assert got[k][:nb].tobytes() == w.tobytes(), f"{what}: {k}"
        assert (got[k][nb:].view(np.uint8) == 7).all(), f"{what}: {k} beyond its rows"


@pytest.mark.parametrize("n", NS)
def test_driver_equals_the_reference(driver, n):
    pack, unpack = driver
    rng = np.random.default_rng(800 + n)
    C, W = n ** 3, ref.words(n ** 3)
    for nb in NBLOCKS:
        for no_infl in ((False, True) if nb in (2, 65) else (False,)):
            what = f"n {n} blocks {nb} no_infl {no_infl}"
            m = wild(rng, cube_keys(rng, nb), C, kinds=None if nb != 65 else np.arange(65) % 9)
            want = ref.pack_rows(m["keys"], m["log_odds"], m["occ"], m["infl"], n, LO_MIN, LO_MAX, no_infl)
            got = pack(m, n, flags=ref.NO_INFL if no_infl else 0)
            assert got["status"] == ref.OK == want["status"], (what, got["text"])
            total = len(want["stream"])
            assert got["stream"][:total] == want["stream"], what
            assert set(got["stream"][total:]) <= {7}, what + ": beyond the stream"
            assert got["summary"].tolist() == want["summary"].tolist(), (what, got["summary"].tolist(), want["summary"].tolist())
            # the summary identities: [1] is the record sizes plus header and directory, [4] is the header's count
            s = want["stream"]
            sizes = [ref.record_bytes(W, *struct.unpack_from("<II", s, 8 * struct.unpack_from("<I", s, ref.HEADER + ref.DIR * i + 12)[0])) for i in range(nb)]
            assert got["summary"][1] == sum(sizes) + ref.HEADER + ref.DIR * nb and got["summary"][4] == struct.unpack_from("<Q", s, 40)[0]
            assert got["summary"][3] == sum(z == 8 for z in sizes)
            # dry, and a null stream: the sizes, nothing written
            for kw in (dict(flags=ref.DRY | (ref.NO_INFL if no_infl else 0)), dict(flags=ref.NO_INFL if no_infl else 0, stream=False)):
                dry = pack(m, n, **kw)
                assert dry["status"] == ref.OK and dry["summary"][:7].tolist() == want["summary"][:7].tolist() and dry["summary"][7] == 0 and set(dry["stream"]) <= {7}, what
            # the round trip: byte for byte the input (infl 'u' where it was left out)
            back = unpack(want["stream"], n, rows_hint=nb)
            assert back["status"] == ref.OK, (what, back["text"])
            expect = dict(m, infl=np.full((nb, C), ref.U, np.uint8)) if no_infl else m
            same_rows(back, expect, nb, what)
            rb = ref.unpack(want["stream"], n)
            assert rb["status"] == ref.OK and all(np.ascontiguousarray(rb[k]).tobytes() == back[k][:nb].tobytes() for k in PLANES), what
            assert back["summary"].tolist() == rb["summary"].tolist(), (what, back["summary"].tolist(), rb["summary"].tolist())


def test_blank_and_special_blocks(driver):
    pack, unpack = driver
    rng = np.random.default_rng(3)
    n, C = 3, 27
    m = wild(rng, cube_keys(rng, 8, bounds=False), C, kinds=[1, 1, 2, 3, 4, 5, 6, 7])
    got = pack(m, n)
    want = ref.pack_rows(m["keys"], m["log_odds"], m["occ"], m["infl"], n, LO_MIN, LO_MAX)
    total = len(want["stream"])
    assert got["stream"][:total] == want["stream"] and got["summary"][3] == 2
    s = want["stream"]
    offs = [struct.unpack_from("<I", s, ref.HEADER + ref.DIR * i + 12)[0] for i in range(8)]
    assert offs[0] == (ref.HEADER + ref.DIR * 8) // 8 and offs[1] == offs[0] + 1 and offs[2] == offs[1] + 1  # a blank block: 8 bytes of record
    assert struct.unpack_from("<II", s, 8 * offs[2]) == (48, 1)  # one -0.0f: val0, val1 and one literal
    assert struct.unpack_from("<II", s, 8 * offs[3]) == (8, 0)   # infl[C-1] 'o': infl1 alone
    assert struct.unpack_from("<II", s, 8 * offs[5]) == (48, C)  # literals only
    assert struct.unpack_from("<II", s, 8 * offs[7]) == (48, 1)
    back = unpack(s, n, rows_hint=8)
    same_rows(back, m, 8, "special")
    assert back["log_odds"].view(np.uint32)[2].max() == 0x80000000 and (back["log_odds"].view(np.uint32)[6] == 0x7FC00001).any()
    # a stream from other clamps decodes to its own bits
    other = ref.pack_rows(m["keys"], m["log_odds"], m["occ"], m["infl"], n, np.float32(0.5), np.float32(9.0))["stream"]
    same_rows(unpack(other, n, rows_hint=8), m, 8, "other clamps")


def small_stream(rng):
    n, C = 2, 8
    m = wild(rng, cube_keys(rng, 5, bounds=False), C, kinds=[0, 1, 3, 5, 7])
    return n, m, ref.pack_rows(m["keys"], m["log_odds"], m["occ"], m["infl"], n, LO_MIN, LO_MAX)["stream"]


def same_verdict(got, want, what):
    assert got["status"] == want["status"], (what, got["status"], got["text"], want)
    if want["status"] != ref.OK:
        assert got["code"] == want["code"] and got["where"] == want["block"] and got["text"] == ref.UNPACK_TEXTS[want["code"]], (what, got["code"], got["where"], want)
        assert not got["summary"].any() and all((got[k].view(np.uint8) == 7).all() for k in PLANES), what
    else:
        nb = len(want["keys"])
        for k in PLANES:
            assert got[k][:nb].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k)
        assert got["summary"].tolist() == want["summary"].tolist(), what


def test_every_single_byte_corruption(driver):
    """every byte of a 5-block stream XOR 0xFF: the driver's verdict, check number, block and output are the reference's"""
    _, unpack = driver
    n, m, s = small_stream(np.random.default_rng(11))
    seen = set()
    for at in range(len(s)):
        bad = bytearray(s)
        bad[at] ^= 0xFF
        want = ref.unpack(bad, n)
        same_verdict(unpack(bad, n, rows_hint=5), want, f"byte {at}")
        seen.add(want.get("code", 0))
    assert {2, 3, 4, 5, 6, 9, 10} <= seen, seen


def test_every_truncation(driver):
    _, unpack = driver
    n, m, s = small_stream(np.random.default_rng(12))
    for length in range(len(s)):
        want = ref.unpack(s[:length], n)
        assert want["status"] == ref.ERR_INVALID and want["code"] == (1 if length < ref.HEADER else 4)
        same_verdict(unpack(s[:length], n, rows_hint=5), want, f"length {length}")
    # bytes behind the total are not the stream's: ignored, never read past
    same_verdict(unpack(s + b"\x55" * 13, n, rows_hint=5), ref.unpack(s, n), "slack")


def test_every_check_number(driver):
    """crafted corruptions that reach the checks a byte flip seldom does: a tail bit (7), a code 3 (8), n_lit off (9), offsets (5), the end (10)"""
    _, unpack = driver
    rng = np.random.default_rng(13)
    n, C = 3, 27
    m = wild(rng, cube_keys(rng, 4, bounds=False), C, kinds=[0, 0, 5, 0])
    s = ref.pack_rows(m["keys"], m["log_odds"], m["occ"], m["infl"], n, LO_MIN, LO_MAX)["stream"]
    offs = [struct.unpack_from("<I", s, ref.HEADER + ref.DIR * i + 12)[0] for i in range(4)]

    def edit(at, fmt, *v):
        b = bytearray(s)
        struct.pack_into(fmt, b, at, *v)
        return b
    pres1 = struct.unpack_from("<I", s, 8 * offs[1])[0]
    assert pres1 & 3 == 3  # occ0 and occ1 present in a wild block
    occ0 = struct.unpack_from("<Q", s, 8 * offs[1] + 8)[0]
    occ1 = struct.unpack_from("<Q", s, 8 * offs[1] + 16)[0]
    free = next(i for i in range(C) if not (occ0 | occ1) >> i & 1)
    cases = [(edit(8 * offs[1] + 8, "<Q", occ0 | 1 << 40), 7, 1), (edit(8 * offs[1] + 8, "<Q", occ0 | 1 << 63), 7, 1),
             (edit(8 * offs[1] + 8, "<QQ", occ0 | 1 << free, occ1 | 1 << free), 8, 1),
             (edit(8 * offs[2] + 4, "<I", C - 2), 9, 2), (edit(8 * offs[2] + 4, "<I", C + 2), 9, 2), (edit(8 * offs[2] + 4, "<I", 1 << 20), 10, 2),
             (edit(ref.HEADER + ref.DIR * 2 + 12, "<I", offs[2] + 1), 5, 2), (edit(ref.HEADER + ref.DIR * 0 + 12, "<I", offs[0] - 1), 5, 0),
             (edit(ref.HEADER + ref.DIR * 3 + 12, "<I", 1 << 31), 5, 3), (edit(8 * offs[0], "<I", 64), 6, 0), (edit(8 * offs[3], "<I", 1 << 31), 6, 3),
             (edit(8, "<I", 64), 3, -1), (edit(12, "<I", 4), 3, -1), (edit(0, "<B", ord("m")), 2, -1), (edit(32, "<Q", len(s) + 8), 4, -1), (edit(32, "<Q", 64), 4, -1),
             (edit(32, "<Q", len(s) - 8), 10, 3), (edit(16, "<I", 3), 5, 0)]
    for bad, code, blk in cases:
        want = ref.unpack(bad, n)
        assert (want["code"], want["block"]) == (code, blk), (code, blk, want)
        same_verdict(unpack(bad, n, rows_hint=4), want, f"check {code} block {blk}")
    # a longer buffer with a total above the records: the last record ends short of it
    want = ref.unpack(edit(32, "<Q", len(s) + 8) + b"\0" * 8, n)
    assert (want["code"], want["block"]) == (10, 3)
    same_verdict(unpack(edit(32, "<Q", len(s) + 8) + b"\0" * 8, n, rows_hint=4), want, "short of the total")


def test_arguments_caps_and_outputs(driver):
    pack, unpack = driver
    rng = np.random.default_rng(14)
    n, C = 2, 8
    m = wild(rng, cube_keys(rng, 5, bounds=False), C)
    want = ref.pack_rows(m["keys"], m["log_odds"], m["occ"], m["infl"], n, LO_MIN, LO_MAX)
    s, total = want["stream"], len(want["stream"])
    box = ([-1, -2, -1], [3, 5, 4])
    bad = [(dict(key_lo=box[0], given=(False,) * 4), 1), (dict(key_dims=box[1], given=(False,) * 4), 1), (dict(key_lo=box[0], key_dims=[1, 0, 1], given=(False,) * 4), 2),
           (dict(key_lo=[0, (1 << 31) - 2, 0], key_dims=[1, 2, 1], given=(False,) * 4), 3), (dict(flags=4), 4), (dict(flags=-1), 4), (dict(key_lo=box[0], key_dims=box[1]), 5),
           (dict(n_arg=-1), 6), (dict(given=(True, False, True, True)), 7), (dict(given=(True, True, False, True)), 7), (dict(misaligned=True), 8)]
    for kw, code in bad:
        got = pack(m, n, **kw)
        assert got["status"] == ref.ERR_INVALID and got["code"] == code and got["text"] == ref.PACK_TEXTS[code], (kw, got)
        assert not got["summary"].any() and set(got["stream"]) <= {7}, kw
    for kw in (dict(key_lo=box[0], key_dims=box[1], given=(False,) * 4), dict(given=(True, True, True, False)), dict(flags=3), dict(n_arg=0)):
        assert pack(m, n, **kw)["status"] == ref.OK, kw
    bare = ref.pack_rows(m["keys"], m["log_odds"], m["occ"], None, n, LO_MIN, LO_MAX)["stream"]
    assert pack(m, n, given=(True, True, True, False))["stream"][:len(bare)] == bare
    # a byte outside 'u' 'f' 'o', in occ and in infl: refused, the row named; with NO_INFL a bad infl byte is not read
    for plane, row in (("occ", 3), ("infl", 1)):
        b = {k: np.array(v, copy=True) for k, v in m.items()}
        b[plane][row, 5] = ord("x")
        b[plane][4, 0] = 0
        got = pack(b, n)
        assert (got["status"], got["code"], got["where"]) == (ref.ERR_INVALID, 9, row) and set(got["stream"]) <= {7} and not got["summary"].any()
        assert ref.pack_rows(b["keys"], b["log_odds"], b["occ"], b["infl"], n, LO_MIN, LO_MAX) == {"status": ref.ERR_INVALID, "code": 9, "row": row}
        assert (pack(b, n, flags=ref.NO_INFL)["status"] == ref.OK) == (plane == "infl")
    # cap_bytes one short: MLM_ERR_CAPACITY, the summary filled, nothing written; exactly enough: fine; a dry call ignores the cap
    short = pack(m, n, cap_bytes=total - 1)
    assert short["status"] == ref.ERR_CAPACITY and short["summary"][:7].tolist() == want["summary"][:7].tolist() and short["summary"][7] == 0 and set(short["stream"]) <= {7}
    assert pack(m, n, cap_bytes=total)["stream"] == s and pack(m, n, cap_bytes=0, flags=ref.DRY)["status"] == ref.OK
    # unpack: arguments, the cap one short, outputs left out in turn, sizing
    for kw, code in ((dict(stream=False), 11), (dict(flags=1), 12), (dict(cap=-1), 13), (dict(misaligned=True), 14)):
        got = unpack(s, n, **{"rows_hint": 5, **kw})
        assert got["status"] == ref.ERR_INVALID and got["code"] == code and got["text"] == ref.UNPACK_TEXTS[code], kw
    rb = ref.unpack(s, n)
    short = unpack(s, n, cap=4)
    assert short["status"] == ref.ERR_CAPACITY and short["summary"][:7].tolist() == rb["summary"][:7].tolist() and all((short[k].view(np.uint8) == 7).all() for k in PLANES)
    sizing = unpack(s, n, cap=0, outputs=0)
    assert sizing["status"] == ref.OK and sizing["summary"][0] == 5 and sizing["summary"][7] == 0
    for skip, k in enumerate(PLANES):
        got = unpack(s, n, cap=5, outputs=15 & ~(1 << skip))
        assert got["status"] == ref.OK and (got[k].view(np.uint8) == 7).all(), k
        for other in PLANES:
            if other != k:
                assert got[other].tobytes() == np.ascontiguousarray(rb[other]).tobytes(), (k, other)
        assert got["summary"][7] == 5 * (12 + 6 * C) - 5 * (12, 4 * C, C, C)[skip]


def test_binding_names_the_calls():
    from mlmapping_amd import mlmap

    assert "mlm_pack_blocks" in mlmap.ABI_SYMBOLS and "mlm_unpack_blocks" in mlmap.ABI_SYMBOLS
    assert (mlmap.MLM_PACK_DRY, mlmap.MLM_PACK_NO_INFL, mlmap.MLM_PACK_ROW) == (ref.DRY, ref.NO_INFL, ref.ROW) == (1, 2, 8)
    assert all(hasattr(mlmap.MLMap, k) for k in ("pack", "unpack", "save", "load"))
    header = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    assert "int mlm_pack_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3]," in header
    assert "int mlm_unpack_blocks(mlm_handle *h, const void *stream, size_t bytes, int flags, int cap," in header
    assert "enum { MLM_PACK_DRY = 1," in header and "MLM_PACK_NO_INFL = 2 };" in header and "#define MLM_PACK_ROW 8" in header
    assert "#define MLM_ABI_VERSION 6" in header
    assert header.index("int mlm_delta_blocks(") < header.index("int mlm_pack_blocks(") < header.index("int mlm_unpack_blocks(") < header.index("int mlm_merge_pack(")
    facade = open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
    assert "mlm_pack_blocks(h_, key_lo, key_dims, n, keys, log_odds, occ, infl, flags, cap_bytes, stream, summary)" in facade
    assert "mlm_unpack_blocks(h_, stream, bytes, flags, cap, keys, log_odds, occ, infl, summary)" in facade
    pack_h = open(os.path.join(CSRC, "mlm_pack.h")).read()
    for name, v in (("F_DRY", 1), ("F_NO_INFL", 2), ("F_ALL", 3), ("SUMS", 8), ("HEADER", 64), ("DIR", 16)):
        assert f"#define MLM_PACK_{name} {v}" in pack_h
    assert '"MLMPACK1"' in pack_h
    for texts, fn in ((ref.PACK_TEXTS, "mlm_pack_check_text"), (ref.UNPACK_TEXTS, "mlm_unpack_check_text")):
        for code, t in texts.items():
            assert f'"{t}"' in pack_h or code in (2, 3, 4), (fn, code)
    assert "mlm_pack_host.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_facade_members_compile(tmp_path):
    """include/mlmap_facade.hpp's packBlocks / unpackBlocks as a C++ client calls them (tests/cpp/pack_client.cpp)"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "pack_client.cpp"),
                           "-o", str(tmp_path / "pack_client.o")])
