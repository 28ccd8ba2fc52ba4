"""mlm_delta_blocks on the CPU: the rule of mlmapping_amd/csrc/mlm_delta.h — argument check, selection, view, digest, join, order — run
as the device phases run it (digest; sort; join; ranks; emission) by tests/cpp/delta_driver.cpp, built with g++
-fsanitize=address,undefined, and held byte for byte to the contract in numpy (tests/delta_ref.py), which is itself held to the
properties the contract states."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import delta_ref as ref
from tests.test_fuse_plan import cube_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
NS = [2, 3, 4, 8]
NBLOCKS = [0, 1, 2, 63, 64, 65, 257]
BOX = ([-1, -2, -1], [3, 5, 4])
PREVS = ("empty", "identical", "subset", "superset", "disjoint")
OUT_ALL = 7


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("delta")
    exe = d / "delta_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "delta_driver.cpp"), "-o", str(exe)])

    def run(m, n, prev=None, key_lo=None, key_dims=None, flags=0, caps=None, outputs=OUT_ALL, n_prev=None, prev_given=None):
        """caps None: room for everything (one row to spare each)"""
        C = n ** 3
        nb = len(m["keys"])
        pk = np.zeros((0, 3), np.int32) if prev is None else np.ascontiguousarray(prev[0], dtype=np.int32).reshape(-1, 3)
        pd = np.zeros((0, 2), np.uint64) if prev is None else np.ascontiguousarray(prev[1], dtype=np.uint64).reshape(-1, 2)
        n_prev = len(pk) if n_prev is None else n_prev
        prev_given = (prev is not None) if prev_given is None else prev_given
        ct, cb, cg = (nb + 1, nb + 1, len(pk) + 1) if caps is None else caps
        lo3 = [0, 0, 0] if key_lo is None else [int(v) for v in key_lo]
        dims3 = [0, 0, 0] if key_dims is None else [int(v) for v in key_dims]
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([nb, n, flags, key_lo is not None, key_dims is not None, *lo3, *dims3, n_prev, int(prev_given), ct, cb, cg, outputs, 0, 0, 0],
                             dtype=np.int64).tobytes())
            for k, dt in (("keys", np.int32), ("log_odds", np.float32), ("occ", np.uint8), ("infl", np.uint8)):
                f.write(np.ascontiguousarray(m[k], dtype=dt).tobytes())
            f.write(np.ascontiguousarray(m.get("collapsed", np.zeros(nb, np.uint8)), dtype=np.uint8).tobytes())
            f.write(pk.tobytes())
            f.write(pd.tobytes())
        subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:128], dtype=np.int64)
        out = {"status": int(head[0]), "code": int(head[1]), "summary": head[2:14].copy(), "text": raw[128:192].split(b"\0")[0].decode()}
        at = 192
        ct, cb, cg = max(ct, 0), max(cb, 0), max(cg, 0)
        for k, dt, rows, cols in (("table_keys", np.int32, ct, 3), ("table_digest", np.uint64, ct, 2), ("keys", np.int32, cb, 3), ("log_odds", np.float32, cb, C),
                                  ("occ", np.uint8, cb, C), ("infl", np.uint8, cb, C), ("kind", np.uint8, cb, 1), ("gone", np.int32, cg, 3)):
            size = rows * cols * np.dtype(dt).itemsize
            out[k] = np.frombuffer(raw[at:at + size], dtype=dt).reshape(rows, cols)
            at += size
        assert at == len(raw)
        return out

    return run


def wild(rng, keys, C, released=False):
    """blocks as anything may have written them, some blank, some blank but for a -0.0f or for their infl, some released"""
    nb = len(keys)
    b = {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": rng.uniform(-3.0, 5.5, size=(nb, C)).astype(np.float32),
         "occ": rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(nb, C)), "infl": rng.choice(np.frombuffer(b"uuo", dtype=np.uint8), size=(nb, C)),
         "collapsed": (rng.random(nb) < 0.2).astype(np.uint8) if released else np.zeros(nb, dtype=np.uint8)}
    kind = rng.random(nb)
    blank = kind < 0.2
    b["log_odds"][blank], b["occ"][blank], b["infl"][blank] = np.float32(0.0), ref.U, ref.U
    b["log_odds"][(kind >= 0.1) & (kind < 0.15), 0] = np.float32(-0.0)
    b["infl"][(kind >= 0.15) & (kind < 0.2), C - 1] = ref.O
    return b


def older(rng, m):
    """the map a while ago: a third of the blocks differ in one bit of one plane of one voxel"""
    old = {k: np.array(v, copy=True) for k, v in m.items()}
    nb, C = old["log_odds"].shape
    changed = np.zeros(nb, dtype=bool)
    for s in np.nonzero(rng.random(nb) < 0.34)[0]:
        c, plane = int(rng.integers(C)), int(rng.integers(3))
        if plane == 0:
            old["log_odds"].view(np.uint32)[s, c] ^= np.uint32(1) << np.uint32(rng.integers(32))
        else:
            old["occ" if plane == 1 else "infl"][s, c] ^= np.uint8(1) << np.uint8(rng.integers(8))
        changed[s] = True
    return old, changed


def table_of(rng, m, extra_keys, which, no_infl):
    """the previous table of a test case, ascending"""
    if which == "empty":
        return None
    old, _ = older(rng, m)
    t = ref.delta(old, no_infl=no_infl)["table"]
    keys, dg = t[0], t[1]
    if which == "subset":
        keep = rng.random(len(keys)) < 0.5
        keys, dg = keys[keep], dg[keep]
    if which in ("superset", "disjoint"):
        ek = np.asarray(extra_keys, dtype=np.int32).reshape(-1, 3)
        ed = rng.integers(0, 1 << 63, size=(len(ek), 2), dtype=np.uint64)
        keys, dg = (ek, ed) if which == "disjoint" else (np.concatenate([keys, ek]), np.concatenate([dg, ed]))
    o = ref.order(keys)
    return keys[o].reshape(-1, 3), dg[o].reshape(-1, 2)


def equal(got, want, names, what):
    """the first rows of every output are the contract's, the rest is untouched"""
    for k in names:
        w = want["table"][0] if k == "table_keys" else want["table"][1] if k == "table_digest" else want[k]
        w = np.ascontiguousarray(w)
        g = got[k]
        assert len(g) >= len(w) and g[:len(w)].tobytes() == w.tobytes(), f"{what}: {k}"
        assert (g[len(w):].view(np.uint8) == 7).all(), f"{what}: {k} beyond its rows"


NAMES = ("table_keys", "table_digest", "keys", "log_odds", "occ", "infl", "kind", "gone")


def untouched(got):
    return all((got[k].view(np.uint8) == 7).all() for k in NAMES)


@pytest.mark.parametrize("n", NS)
def test_driver_equals_the_reference(driver, n):
    rng = np.random.default_rng(700 + n)
    C = n ** 3
    seen = {"changed": 0, "new": 0, "gone": 0, "unchanged": 0, "ignored": 0}
    for nb in NBLOCKS:
        allk = cube_keys(rng, nb + 9)
        m = wild(rng, allk[:nb], C, released=(n == 3))
        for which in PREVS:
            combos = list(itertools.product((False, True), (False, True))) if nb in (65, 257) else [(False, False), (True, True)]
            for box, no_infl in combos:
                what = f"n {n} blocks {nb} prev {which} box {box} no_infl {no_infl}"
                prev = table_of(rng, m, allk[nb:], which, no_infl)
                lo, dims = BOX if box else (None, None)
                want = ref.delta(m, prev, lo, dims, no_infl)
                flags = ref.NO_INFL if no_infl else 0
                got = driver(m, n, prev, lo, dims, flags)
                assert got["status"] == ref.OK == want["status"] and got["code"] == 0, what
                assert got["summary"].tolist() == want["summary"].tolist(), (what, got["summary"].tolist(), want["summary"].tolist())
                equal(got, want, NAMES, what)
                sm = want["summary"]
                assert sm[1] == sm[4] + sm[5] + sm[6] and sm[3] == sm[4] + sm[5] + sm[7], what
                # the new table is a valid previous table: the call against it finds nothing
                again = driver(m, n, want["table"], lo, dims, flags)
                assert again["status"] == ref.OK and again["summary"][4] == sm[1] and not again["summary"][5:9].any(), what
                # dry: the counts, and nothing written
                dry = driver(m, n, prev, lo, dims, flags | ref.DRY)
                assert dry["status"] == ref.OK and dry["summary"][:8].tolist() == sm[:8].tolist() and not dry["summary"][8:11].any() and dry["summary"][11] == sm[11], what
                assert untouched(dry), what
                seen["changed"] += int(sm[5]); seen["new"] += int(sm[6]); seen["gone"] += int(sm[7]); seen["unchanged"] += int(sm[4]); seen["ignored"] += int(sm[2] - sm[3])
    assert all(v > 0 for v in seen.values()), seen


def test_outputs_left_out_and_capacity(driver):
    rng = np.random.default_rng(31)
    n, C, nb = 2, 8, 65
    allk = cube_keys(rng, nb + 9)
    m = wild(rng, allk[:nb], C)
    prev = table_of(rng, m, allk[nb:], "superset", False)
    want = ref.delta(m, prev)
    sm = want["summary"]
    S, E, G = int(sm[1]), int(sm[5] + sm[6]), int(sm[7])
    assert S == nb and 0 < E < S and G == 9
    for outputs, names in ((1, NAMES[:2]), (2, NAMES[2:7]), (4, NAMES[7:]), (0, ())):
        got = driver(m, n, prev, outputs=outputs, caps=(S, E, G) if outputs else (0, 0, 0))
        assert got["status"] == ref.OK, outputs
        equal(got, want, names, f"outputs {outputs}")
        assert all((got[k].view(np.uint8) == 7).all() for k in NAMES if k not in names)
        assert got["summary"][:8].tolist() == sm[:8].tolist()
        assert got["summary"][8:11].tolist() == [E if outputs & 2 else 0, S if outputs & 1 else 0, G if outputs & 4 else 0]
    # each cap one short: MLM_ERR_CAPACITY, the summary filled, the outputs untouched; a cap whose outputs are left out does not count
    for caps, outputs in (((S - 1, E, G), 1), ((S, E - 1, G), 2), ((S, E, G - 1), 4)):
        got = driver(m, n, prev, caps=caps)
        assert got["status"] == ref.ERR_CAPACITY and ref.capacity_short(sm, *caps) and untouched(got), caps
        assert got["summary"][:8].tolist() == sm[:8].tolist() and not got["summary"][8:11].any() and got["summary"][11] == sm[11]
        assert driver(m, n, prev, caps=caps, outputs=OUT_ALL & ~outputs)["status"] == ref.OK
        assert not ref.capacity_short(sm, *caps, table_out=outputs != 1, block_out=outputs != 2, gone_out=outputs != 4)
    assert not ref.capacity_short(sm, S, E, G)


def flips(lo, occ, infl):
    """every single-bit flip of the three planes of one block, and every swap of two unequal cells"""
    C = lo.shape[1]
    out = []
    for c in range(C):
        for bit in range(32):
            v = lo.copy()
            v.view(np.uint32)[0, c] ^= np.uint32(1) << np.uint32(bit)
            out.append(("lo", v, occ, infl))
        for bit in range(8):
            v = occ.copy()
            v[0, c] ^= np.uint8(1 << bit)
            out.append(("occ", lo, v, infl))
            v = infl.copy()
            v[0, c] ^= np.uint8(1 << bit)
            out.append(("infl", lo, occ, v))
    n_flips = len(out)
    for a, b in itertools.combinations(range(C), 2):
        if (lo.view(np.uint32)[0, a], occ[0, a], infl[0, a]) != (lo.view(np.uint32)[0, b], occ[0, b], infl[0, b]):
            p = np.arange(C)
            p[[a, b]] = [b, a]
            out.append(("swap", lo[:, p], occ[:, p], infl[:, p]))
    return out, n_flips


@pytest.mark.parametrize("C", [8, 27])
def test_digest_properties(C):
    rng = np.random.default_rng(90 + C)
    b = wild(rng, np.zeros((1, 3), np.int32), C)
    b["log_odds"][:] = rng.uniform(-3.0, 5.5, size=(1, C)).astype(np.float32)
    b["occ"][:] = rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(1, C))
    lo, occ, infl = b["log_odds"], b["occ"], b["infl"]
    variants, n_flips = flips(lo, occ, infl)
    assert n_flips == 48 * C  # (384 and 1 296)
    base = ref.digest(lo, occ, infl)[0]
    dgs = np.array([ref.digest(*v[1:])[0] for v in variants], dtype=np.uint64)
    assert (dgs[:, 0] != base[0]).all() and (dgs[:, 1] != base[1]).all()
    assert len(set(dgs[:, 0].tolist()) | {int(base[0])}) == len(variants) + 1  # pairwise distinct in d[0] already
    # with MLM_DELTA_NO_INFL an infl flip does not change the digest, anything else still does
    for what, l, o, i in variants:
        v = {"keys": b["keys"], "log_odds": l, "occ": o, "infl": i}
        same = ref.digest(*ref.view(v, no_infl=True)).tobytes() == ref.digest(*ref.view(b, no_infl=True)).tobytes()
        assert same == (what == "infl"), what
    # -0.0f and +0.0f differ
    z = lo.copy()
    z[0, 0] = np.float32(0.0)
    mz = z.copy()
    mz[0, 0] = np.float32(-0.0)
    assert ref.digest(z, occ, infl).tobytes() != ref.digest(mz, occ, infl).tobytes()


def test_blank_block_pins_the_constants(driver):
    blank = {"keys": np.zeros((1, 3), np.int32), "log_odds": np.zeros((1, 8), np.float32), "occ": np.full((1, 8), ref.U, np.uint8), "infl": np.full((1, 8), ref.U, np.uint8)}
    assert tuple(int(x) for x in ref.digest(blank["log_odds"], blank["occ"], blank["infl"])[0]) == ref.BLANK8 == (0xaa5d834bd09a229e, 0x71cf1fe0a9b5a6df)
    got = driver(blank, 2)
    assert got["status"] == ref.OK and tuple(int(x) for x in got["table_digest"][0]) == ref.BLANK8
    assert got["summary"].tolist() == [1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1]
    # a released block of any content reads as its element 0 with infl 'u'
    rng = np.random.default_rng(5)
    b = wild(rng, np.zeros((1, 3), np.int32), 27)
    b["collapsed"][:] = 1
    flat = {k: np.array(v, copy=True) for k, v in b.items()}
    flat["log_odds"][:] = b["log_odds"][0, 0]
    flat["occ"][:] = b["occ"][0, 0]
    flat["infl"][:] = ref.U
    flat["collapsed"][:] = 0
    a, c = driver(b, 3), driver(flat, 3)
    assert a["table_digest"][:1].tobytes() == c["table_digest"][:1].tobytes() == ref.delta(flat)["table"][1].tobytes() == ref.delta(b)["table"][1].tobytes()
    for k in ("log_odds", "occ", "infl"):
        assert a[k].tobytes() == c[k].tobytes()


def test_argument_check(driver):
    rng = np.random.default_rng(1)
    m = wild(rng, cube_keys(rng, 5, bounds=False), 8)
    prev = ref.delta(m)["table"]
    lo, dims = BOX
    big = 1 << 20
    bad_range = (np.concatenate([prev[0], [[big, 0, 0]]]).astype(np.int32), np.concatenate([prev[1], [[1, 2]]]).astype(np.uint64))
    low_range = (np.concatenate([[[0, -big - 1, 0]], prev[0]]).astype(np.int32), np.concatenate([[[1, 2]], prev[1]]).astype(np.uint64))
    swapped = (prev[0][[1, 0, 2, 3, 4]], prev[1][[1, 0, 2, 3, 4]])
    twice = (prev[0][[0, 1, 1, 2, 3]], prev[1][[0, 1, 1, 2, 3]])
    cases = [(dict(key_lo=lo), 1), (dict(key_dims=dims), 1), (dict(key_lo=lo, key_dims=[1, 0, 1]), 2), (dict(key_lo=lo, key_dims=[1, 1, -5]), 2),
             (dict(key_lo=[0, (1 << 31) - 2, 0], key_dims=[1, 2, 1]), 3), (dict(flags=4), 4), (dict(flags=-1), 4), (dict(flags=1 << 30), 4),
             (dict(caps=(-1, 9, 9)), 5), (dict(caps=(9, -1, 9)), 5), (dict(caps=(9, 9, -1)), 5), (dict(n_prev=-1), 5), (dict(n_prev=3, prev_given=False), 6),
             (dict(prev=bad_range), 7), (dict(prev=low_range), 7), (dict(prev=swapped), 8), (dict(prev=twice), 8),
             (dict(), 0), (dict(key_lo=lo, key_dims=dims), 0), (dict(prev=prev), 0), (dict(flags=3), 0), (dict(key_lo=[0, (1 << 31) - 2, 0], key_dims=[1, 1, 1]), 0)]
    for case, code in cases:
        got = driver(m, 2, **case)
        assert got["code"] == code and got["status"] == (ref.ERR_INVALID if code else ref.OK), (case, got["code"])
        if code:
            assert got["text"] == ref.TEXTS[code], case
            assert not got["summary"].any() and untouched(got), case
        if code in (7, 8):
            assert ref.delta(m, case["prev"])["code"] == code
        elif "caps" not in case and "n_prev" not in case:
            p = case.get("prev")
            assert ref.check_args(case.get("key_lo"), case.get("key_dims"), 0 if p is None else len(p[0]), True, case.get("flags", 0)) == code, case
    assert ref.check_args(None, None, -1, True, 0) == 5 and ref.check_args(None, None, 0, True, 0, cap_gone=-1) == 5 and ref.check_args(None, None, 3, False, 0) == 6
    # the box errors carry mlm_crop_blocks' texts
    crop_h = open(os.path.join(CSRC, "mlm_crop.h")).read()
    assert all(f'"{ref.TEXTS[k]}"' in crop_h for k in (2, 3, 4))


def test_binding_names_the_call():
    from mlmapping_amd import mlmap

    assert "mlm_delta_blocks" in mlmap.ABI_SYMBOLS
    assert (mlmap.MLM_DELTA_DRY, mlmap.MLM_DELTA_NO_INFL, mlmap.MLM_DELTA_ROW) == (ref.DRY, ref.NO_INFL, ref.ROW) == (1, 2, 12)
    assert all(hasattr(mlmap.MLMap, k) for k in ("delta", "apply_delta"))
    header = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    assert "int mlm_delta_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3]," in header
    assert "enum { MLM_DELTA_DRY = 1," in header and "MLM_DELTA_NO_INFL = 2 };" in header and "#define MLM_DELTA_ROW 12" in header
    assert "#define MLM_ABI_VERSION 6" in header
    assert header.index("int mlm_age_blocks(") < header.index("int mlm_delta_blocks(") < header.index("int mlm_merge_pack(")
    assert "A changed block is missed with probability about 2^-128 per comparison." in " ".join(header.replace(" * ", " ").split())
    facade = open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
    assert "mlm_delta_blocks(h_, key_lo, key_dims, n_prev, prev_keys, prev_digest, flags, cap_table, cur_keys, cur_digest, cap, keys," in facade
    delta_h = open(os.path.join(CSRC, "mlm_delta.h")).read()
    for name, v in (("F_DRY", 1), ("F_NO_INFL", 2), ("F_ALL", 3), ("SUMS", 12), ("K_CHANGED", 1), ("K_NEW", 2)):
        assert f"#define MLM_DELTA_{name} {v}" in delta_h
    assert "0x9E3779B97F4A7C15" in delta_h and "0xBF58476D1CE4E5B9" in delta_h and "0x94D049BB133111EB" in delta_h and "0xD6E8FEB86659FD93" in delta_h


def test_facade_member_compiles(tmp_path):
    """include/mlmap_facade.hpp's deltaBlocks as a C++ client calls it (tests/cpp/delta_client.cpp)"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "delta_client.cpp"),
                           "-o", str(tmp_path / "delta_client.o")])
