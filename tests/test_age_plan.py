"""mlm_age_blocks on the CPU: the rule of mlmapping_amd/csrc/mlm_age.h — argument check, selection, the per-voxel rule with its counts,
the empty-block predicate — and mlm_crop.h's hole filling over the empty blocks, run as the device phases run them (apply and block
states; count / scan / rank; move; tail reset) by tests/cpp/age_driver.cpp, built with g++ -fsanitize=address,undefined, and held byte for
byte to the contract in numpy (tests/age_ref.py), which is itself held to the properties the contract states."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import age_ref as ref
from tests.test_fuse_plan import cube_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
NS = [2, 3, 4, 8]
NBLOCKS = [0, 1, 2, 63, 64, 65, 257, 2049]
PLANES = ("keys", "log_odds", "occ", "infl")
LO_MIN, LO_MAX, SH = (np.float32(v) for v in ref.LIMITS)
AMOUNT = {ref.SCALE: np.float32(0.5), ref.STEP: np.float32(0.375)}
FORGET = np.float32(0.25)
BOX = ([-1, -2, -1], [3, 5, 4])
FLAG_BITS = (ref.OUTSIDE, ref.DRY, ref.FORGET, ref.DROP, ref.CLEAR_INFL)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("age")
    exe = d / "age_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "age_driver.cpp"), "-o", str(exe)])

    def run(m, n, key_lo=None, key_dims=None, mode=ref.SCALE, amount=1.0, forget=0.0, flags=0, per_block=True, lim=ref.LIMITS):
        C = n ** 3
        nb = len(m["keys"])
        lo3 = [0, 0, 0] if key_lo is None else [int(v) for v in key_lo]
        dims3 = [0, 0, 0] if key_dims is None else [int(v) for v in key_dims]
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([nb, n, mode, flags, key_lo is not None, key_dims is not None, *lo3, *dims3, int(per_block), 0, 0, 0], dtype=np.int64).tobytes())
            f.write(np.array([*lim, amount, forget], dtype=np.float32).tobytes())
            for k, dt in (("keys", np.int32), ("log_odds", np.float32), ("occ", np.uint8), ("infl", np.uint8)):
                f.write(np.ascontiguousarray(m[k], dtype=dt).tobytes())
        subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:128], dtype=np.int64)
        text = raw[128:192].split(b"\0")[0].decode()
        nb2, pr, at = int(head[14]), int(head[15]), 192
        out = {"per_block": np.frombuffer(raw[at:at + pr * 16], dtype=np.int32).reshape(pr, 4)}
        at += pr * 16
        for k, dt, cols in (("keys", np.int32, 3), ("log_odds", np.float32, C), ("occ", np.uint8, C), ("infl", np.uint8, C)):
            size = nb2 * cols * np.dtype(dt).itemsize
            out[k] = np.frombuffer(raw[at:at + size], dtype=dt).reshape(nb2, cols)
            at += size
        assert at == len(raw)
        out.update(status=int(head[0]), code=int(head[1]), text=text, summary=head[2:14].copy())
        return out

    return run


def values(rng, shape):
    """log-odds in and beyond the clamp range; exactly occupied_sh, log_odds_min, log_odds_max, +-forget, +-both amounts, +-0.0; a NaN;
    subnormals, and a normal value that SCALE by 0.5 makes subnormal"""
    v = rng.uniform(-3.0, 5.5, size=shape).astype(np.float32)
    special = [SH, LO_MIN, LO_MAX, FORGET, -FORGET, AMOUNT[ref.SCALE], -AMOUNT[ref.SCALE], AMOUNT[ref.STEP], -AMOUNT[ref.STEP], np.float32(0.0), np.float32(-0.0),
               np.float32(np.nan), np.float32(1e-40), np.float32(-1e-40), np.float32(1.5e-38), np.float32(-1.5e-38), np.float32(0.1), np.float32(-0.2),
               np.float32(2 * FORGET), np.float32(FORGET + AMOUNT[ref.STEP]), np.float32(np.inf), np.float32(-np.inf)]
    pick = rng.integers(0, 3 * len(special), size=shape)
    for j, x in enumerate(special):
        v[pick == j] = x
    return v


def wild(rng, keys, C):
    """a map as anything may have written it: classes and log-odds unrelated, evidence-only voxels ('u' with nonzero log-odds), blocks
    nothing has touched (already empty), blocks of small values only (they empty out under FORGET), blocks empty but for their infl"""
    nb = len(keys)
    b = {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": values(rng, (nb, C)),
         "occ": rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(nb, C)), "infl": rng.choice(np.frombuffer(b"uuo", dtype=np.uint8), size=(nb, C))}
    kind = rng.random(nb)
    blank = kind < 0.15
    b["log_odds"][blank], b["occ"][blank], b["infl"][blank] = np.float32(0.0), ref.U, ref.U
    small = (kind >= 0.15) & (kind < 0.35)
    b["log_odds"][small] = rng.uniform(-0.3, 0.3, size=(int(small.sum()), C)).astype(np.float32)
    b["infl"][small] = ref.U
    halo = (kind >= 0.35) & (kind < 0.45)
    b["log_odds"][halo], b["occ"][halo] = np.float32(-0.0), ref.U
    return b


def same(a, b, what=""):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def kwargs_of(flags, mode, box=True):
    """age_ref.age's arguments of a flag word"""
    return dict(key_lo=BOX[0] if box else None, key_dims=BOX[1] if box else None, mode=mode, amount=AMOUNT[mode], forget=FORGET if flags & ref.FORGET else None,
                outside=bool(flags & ref.OUTSIDE), drop=bool(flags & ref.DROP), clear_infl=bool(flags & ref.CLEAR_INFL), dry=bool(flags & ref.DRY))


def check_properties(m, want, sm, pr, flags, what):
    """what the contract states of any call, held on the reference's own answer"""
    nb = len(m["keys"])
    assert sm[0] == nb and sm[3] == nb - sm[2] and sm[6] >= sm[7] + sm[8] and sm[1] == int((pr[:, 3] != 0).sum()), what
    assert pr[:, 0].sum() == sm[4] and pr[:, 1].sum() == sm[6] and pr[:, 2].sum() == sm[9] + sm[10], what
    assert sm[2] == (int((pr[:, 3] == 2).sum()) if flags & ref.DROP else 0), what
    if flags & ref.DRY:
        same(want, m, what)
    elif flags & ref.DROP:  # every dropped block was empty, and no selected block that is still there is
        assert len(want["keys"]) == sm[3], what
        left = {tuple(k) for k in want["keys"].tolist()}
        gone = np.array([tuple(k) not in left for k in m["keys"].tolist()], dtype=bool).reshape(nb)
        assert np.array_equal(gone, pr[:, 3] == 2), what
        kept_sel = {tuple(k) for k in m["keys"][pr[:, 3] == 1].tolist()}
        still = np.array([tuple(k) in kept_sel for k in want["keys"].tolist()], dtype=bool).reshape(len(want["keys"]))
        assert not ref.empty_blocks(want)[still].any(), what
    else:
        assert np.array_equal(want["keys"], m["keys"]), what
    if not flags & ref.FORGET:
        assert sm[6] == sm[7] == sm[8] == 0, what
    if not flags & ref.CLEAR_INFL:
        assert sm[11] == 0, what


@pytest.mark.parametrize("n", NS)
def test_driver_equals_the_reference(driver, n):
    rng = np.random.default_rng(200 + n)
    C = n ** 3
    seen_flags = set()
    for nb in NBLOCKS:
        m = wild(rng, cube_keys(rng, nb, bounds=False) if nb else np.zeros((0, 3), np.int32), C)
        # every flag combination at 65 blocks; elsewhere the combinations that take another path
        combos = range(32) if nb == 65 else (0, ref.DRY | ref.FORGET | ref.DROP, ref.FORGET | ref.DROP, ref.OUTSIDE | ref.FORGET | ref.DROP | ref.CLEAR_INFL)
        for flags, mode, box in itertools.product(combos, (ref.SCALE, ref.STEP), (True, False)):
            if not box and nb not in (65, 257):
                continue
            what = f"n {n} blocks {nb} flags {flags} mode {mode} box {box}"
            kw = kwargs_of(flags, mode, box)
            want, sm, pr = ref.age(m, **kw)
            got = driver(m, n, kw["key_lo"], kw["key_dims"], mode, AMOUNT[mode], FORGET, flags)
            assert got["status"] == ref.OK and got["code"] == 0, what
            same(got, want, what)
            assert got["summary"].tolist() == sm.tolist(), (what, got["summary"].tolist(), sm.tolist())
            assert got["per_block"].tolist() == pr.tolist(), what
            check_properties(m, want, sm, pr, flags, what)
            if flags & ref.DRY:  # the counts of the call without it
                _, sm_wet, pr_wet = ref.age(m, **dict(kw, dry=False))
                assert sm.tolist() == sm_wet.tolist() and pr.tolist() == pr_wet.tolist(), what
            if nb >= 63 and box:
                assert 0 < sm[1] < nb, what
            if nb >= 63 and (flags & ref.FORGET) and (flags & ref.DROP):
                assert sm[2] > 0 and sm[6] > sm[7] + sm[8] > 0, what
            seen_flags.add(flags)
    assert seen_flags == set(range(32))


@pytest.mark.parametrize("n", [2, 3])
def test_properties_of_the_rule(driver, n):
    rng = np.random.default_rng(60 + n)
    C = n ** 3
    m = wild(rng, cube_keys(rng, 257, bounds=False), C)
    # SCALE by 1 with no other flag is the identity — on values inside the clamp range (beyond it the clamp acts, and a NaN becomes log_odds_min)
    tame = {k: v.copy() for k, v in m.items()}
    with np.errstate(invalid="ignore"):
        tame["log_odds"] = np.where(np.isnan(m["log_odds"]), np.float32(0.5), ref.clamp(m["log_odds"], ref.LIMITS)).astype(np.float32)
    # ... and classes as the class rule leaves them, or the rule would set them
    cls = np.where(tame["log_odds"] > SH, ref.O, ref.F).astype(np.uint8)
    tame["occ"] = np.where(tame["occ"] == ref.U, ref.U, cls).astype(np.uint8)
    after, sm, pr = ref.age(tame, mode=ref.SCALE, amount=1.0)
    same(after, tame, "identity")
    assert sm[4] > 0 and not sm[5:].any() and sm[2] == 0 and not pr[:, 1:3].any()
    got = driver(tame, n, mode=ref.SCALE, amount=1.0)
    same(got, tame, "driver identity")
    assert got["summary"].tolist() == sm.tolist()
    # subnormals are kept: 1e-40f survives SCALE by 1 and halves under SCALE by 0.5; 1.5e-38f becomes the subnormal 0.75e-38f
    tiny = {k: v[:1].copy() for k, v in m.items()}
    tiny["log_odds"][0, :4] = np.array([1e-40, -1e-40, 1.5e-38, -1.5e-38], dtype=np.float32)
    tiny["occ"][0, :4] = np.frombuffer(b"ufou", dtype=np.uint8)
    halves = (tiny["log_odds"][0, :4].astype(np.float64) / 2).astype(np.float32)
    for a in (ref.age(tiny, mode=ref.SCALE, amount=0.5)[0], driver(tiny, n, mode=ref.SCALE, amount=0.5)):
        got4 = a["log_odds"][0, :4]
        assert got4.view(np.uint32).tolist() == halves.view(np.uint32).tolist()
        assert (got4 != 0).all() and (np.abs(got4) < np.finfo(np.float32).tiny).all()
        assert a["occ"][0, :4].tobytes() == b"uffu"  # (0.75e-38 <= occupied_sh: 'o' turns 'f'; evidence only stays 'u')
    # STEP never changes a sign, never crosses zero and never grows a magnitude
    for amount in (0.0, 0.375, 1.0, 10.0):
        after, sm, _ = ref.age(tame, mode=ref.STEP, amount=amount)
        a, b = tame["log_odds"], after["log_odds"]
        assert not ((a > 0) & (b < 0)).any() and not ((a < 0) & (b > 0)).any() and (np.abs(b) <= np.abs(a)).all()
        got = driver(tame, n, mode=ref.STEP, amount=amount)
        same(got, after, f"driver step {amount}")
        assert got["summary"].tolist() == sm.tolist()
    # two SCALE calls by 0.5 equal one by 0.25 (a power of two: both exact on normal values)
    half, _, _ = ref.age(tame, mode=ref.SCALE, amount=0.5)
    twice, _, _ = ref.age(half, mode=ref.SCALE, amount=0.5)
    once, _, _ = ref.age(tame, mode=ref.SCALE, amount=0.25)
    normal = (np.abs(tame["log_odds"]) >= np.float32(1e-30)) | (tame["log_odds"] == 0)
    assert np.array_equal(twice["log_odds"].view(np.uint32)[normal], once["log_odds"].view(np.uint32)[normal])
    assert np.array_equal(twice["occ"][normal], once["occ"][normal])
    # aging never classifies: a voxel that was 'u' stays 'u', in every mode, forgetting or not
    for mode in (ref.SCALE, ref.STEP):
        for forget in (None, FORGET):
            after, sm, _ = ref.age(m, mode=mode, amount=AMOUNT[mode], forget=forget)
            assert (after["occ"][m["occ"] == ref.U] == ref.U).all() and np.isfinite(after["log_odds"][m["occ"] != ref.U]).all()
            assert np.array_equal(after["infl"], m["infl"])
    # a -0.0f / 'u' voxel and allocate_ram's 0.0f / 'u' keep their bits; CLEAR_INFL clears every voxel of a selected block, aged or not
    after, sm, _ = ref.age(m, mode=ref.SCALE, amount=0.0, clear_infl=True)
    idle = (m["occ"] == ref.U) & ~ref.has_evidence(m["log_odds"])
    assert np.array_equal(after["log_odds"].view(np.uint32)[idle], m["log_odds"].view(np.uint32)[idle]) and (m["log_odds"].view(np.uint32)[idle] != 0).any()
    assert (after["infl"] == ref.U).all() and sm[11] == int((m["infl"] == ref.O).sum()) > 0
    got = driver(m, n, mode=ref.SCALE, amount=0.0, flags=ref.CLEAR_INFL)
    same(got, after, "driver clear_infl")
    # a negative occupied_sh: STEP can turn 'f' into 'o'
    lim = (-2.0, 4.2, -0.5)
    f_lo = {k: v.copy() for k, v in tame.items()}
    f_lo["occ"] = np.where(f_lo["occ"] == ref.U, ref.U, np.where(f_lo["log_odds"] > np.float32(-0.5), ref.O, ref.F)).astype(np.uint8)
    after, sm, pr = ref.age(f_lo, mode=ref.STEP, amount=0.375, lim=lim)
    assert sm[10] > 0 and sm[9] == 0 and pr[:, 2].sum() == sm[10]
    got = driver(f_lo, n, mode=ref.STEP, amount=0.375, lim=lim)
    same(got, after, "driver negative threshold")
    assert got["summary"].tolist() == sm.tolist()


def test_drop_is_the_crop_of_the_empty_blocks(driver):
    """the slot order after a DROP is crop_ref's hole filling over the empty selected blocks of the call without DROP"""
    from tests import crop_ref

    rng = np.random.default_rng(9)
    n, C = 2, 8
    m = wild(rng, cube_keys(rng, 4097, bounds=False), C)  # (more than two chunks of the prefix)
    plain, sm0, pr0 = ref.age(m, *BOX, mode=ref.STEP, amount=0.375, forget=FORGET, outside=True)
    want, sm, pr = ref.age(m, *BOX, mode=ref.STEP, amount=0.375, forget=FORGET, outside=True, drop=True)
    p = crop_ref.plan(pr0[:, 3] == 2)
    assert p["D"] == sm[2] > 100 and p["H"] > 10 and pr.tolist() == pr0.tolist()
    same(want, {k: plain[k][p["order"]] for k in PLANES}, "by the definition")
    got = driver(m, n, *BOX, ref.STEP, 0.375, FORGET, ref.OUTSIDE | ref.FORGET | ref.DROP)
    same(got, want, "driver")
    assert got["summary"].tolist() == sm.tolist() and got["per_block"].tolist() == pr.tolist()


INVALID = [(dict(key_dims=None), 1), (dict(key_lo=None), 1), (dict(key_dims=[1, 0, 1]), 2), (dict(key_dims=[1, 1, -5]), 2),
           (dict(key_lo=[0, (1 << 31) - 2, 0], key_dims=[1, 2, 1]), 3), (dict(flags=32), 4), (dict(flags=-1), 4), (dict(flags=1 << 30), 4),
           (dict(mode=2), 5), (dict(mode=-1), 5), (dict(amount=np.nan), 6), (dict(amount=np.inf), 6), (dict(mode=ref.STEP, amount=-np.inf), 6),
           (dict(amount=1.5), 7), (dict(amount=-0.25), 7), (dict(mode=ref.STEP, amount=-0.25), 8),
           (dict(flags=ref.FORGET, forget=-0.5), 9), (dict(flags=ref.FORGET, forget=np.nan), 9), (dict(flags=ref.FORGET | ref.DRY, forget=np.inf), 9)]
VALID = [dict(), dict(key_lo=None, key_dims=None), dict(forget=np.nan), dict(forget=-1.0), dict(mode=ref.STEP, amount=7.0), dict(amount=0.0), dict(amount=1.0),
         dict(flags=31, forget=0.0), dict(key_lo=[0, (1 << 31) - 2, 0], key_dims=[1, 1, 1]), dict(per_block=False)]


def test_argument_check(driver):
    rng = np.random.default_rng(1)
    m = wild(rng, cube_keys(rng, 5, bounds=False), 8)
    for case, code in INVALID + [(c, 0) for c in VALID]:
        a = dict(key_lo=BOX[0], key_dims=BOX[1], mode=ref.SCALE, amount=0.5, forget=0.0, flags=0, per_block=True)
        a.update(case)
        assert ref.check_args(a["key_lo"], a["key_dims"], a["mode"], a["amount"], a["forget"], a["flags"]) == code, case
        got = driver(m, 2, **a)
        assert got["code"] == code and got["status"] == (ref.ERR_INVALID if code else ref.OK), (case, got["code"])
        if code:
            assert got["text"] == ref.TEXTS[code], case
            assert not got["summary"].any() and len(got["per_block"]) == 0
            same(got, m, str(case))
    # the box errors carry mlm_crop_blocks' texts
    crop_h = open(os.path.join(CSRC, "mlm_crop.h")).read()
    assert all(f'"{ref.TEXTS[k]}"' in crop_h for k in (2, 3, 4))


def test_binding_names_the_call():
    from mlmapping_amd import mlmap

    assert "mlm_age_blocks" in mlmap.ABI_SYMBOLS
    assert (mlmap.MLM_AGE_SCALE, mlmap.MLM_AGE_STEP) == (ref.SCALE, ref.STEP) and mlmap.AGE_MODES == ref.MODES
    assert (mlmap.MLM_AGE_OUTSIDE, mlmap.MLM_AGE_DRY, mlmap.MLM_AGE_FORGET, mlmap.MLM_AGE_DROP, mlmap.MLM_AGE_CLEAR_INFL) == FLAG_BITS == (1, 2, 4, 8, 16)
    assert (mlmap.MLM_AGE_ROW, mlmap.MLM_AGE_COLS) == (ref.ROW, ref.COLS)
    assert all(hasattr(mlmap.MLMap, k) for k in ("age_blocks", "age_outside", "retain_box", "retain_around"))
    header = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    assert "int mlm_age_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int mode, float amount, float forget," in header
    assert "enum { MLM_AGE_SCALE = 0, MLM_AGE_STEP = 1 };" in header and "#define MLM_AGE_ROW 12" in header and "#define MLM_AGE_COLS 4" in header
    assert "enum { MLM_AGE_OUTSIDE = 1, MLM_AGE_DRY = 2, MLM_AGE_FORGET = 4," in header and "MLM_AGE_DROP = 8, MLM_AGE_CLEAR_INFL = 16 };" in header
    assert "#define MLM_ABI_VERSION 6" in header
    assert header.index("int mlm_fuse_blocks(") < header.index("int mlm_age_blocks(") < header.index("int mlm_merge_pack(")
    assert "mlm_age_blocks(h_, key_lo, key_dims, mode, amount, forget, flags, per_block, summary)" in open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
    age_h = open(os.path.join(CSRC, "mlm_age.h")).read()
    for name, v in (("M_SCALE", 0), ("M_STEP", 1), ("F_OUTSIDE", 1), ("F_DRY", 2), ("F_FORGET", 4), ("F_DROP", 8), ("F_CLEAR_INFL", 16), ("F_ALL", 31),
                    ("SUMS", 12), ("PB", 4)):
        assert f"#define MLM_AGE_{name} {v}" in age_h


def test_facade_member_compiles(tmp_path):
    """include/mlmap_facade.hpp's ageBlocks as a C++ client calls it (tests/cpp/age_client.cpp)"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "age_client.cpp"),
                           "-o", str(tmp_path / "age_client.o")])
