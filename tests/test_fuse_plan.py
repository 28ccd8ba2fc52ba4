"""mlm_fuse_blocks on the CPU: the rule of mlmapping_amd/csrc/mlm_fuse.h — argument check, key checks, touch and create predicates, the
per-voxel rule and its counts — run as the device phases run it (probe, duplicate check, rank, create, apply) by
tests/cpp/fuse_driver.cpp, built with g++ -fsanitize=address,undefined, and held byte for byte to the contract in numpy
(tests/fuse_ref.py), which is itself held to the properties the contract states."""
import os
import subprocess

import numpy as np
import pytest

from tests import fuse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
NS = [2, 3, 4, 8]
NROWS = [0, 1, 2, 63, 64, 65, 257]
PLANES = ("keys", "log_odds", "occ", "infl")
LO_MIN, LO_MAX, SH = (np.float32(v) for v in ref.LIMITS)
BOUND_KEYS = np.array([[ref.KEY_MAX, 0, 0], [ref.KEY_MIN, ref.KEY_MIN, ref.KEY_MIN], [0, ref.KEY_MAX, ref.KEY_MIN], [-1, ref.KEY_MIN, ref.KEY_MAX]], dtype=np.int32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("fuse")
    exe = d / "fuse_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "fuse_driver.cpp"), "-o", str(exe)])

    def run(m, rows, n, mode=ref.ADD, flags=0, infl_given=True, per_row=True, rows_n=None, null=(), cap=0, grow=True):
        C = n ** 3
        nb, nr = len(m["keys"]), len(rows["keys"])
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([nb, n, nr if rows_n is None else rows_n, mode, flags, int(infl_given), "keys" in null, "log_odds" in null, "occ" in null,
                              int(per_row), cap, int(grow), 0, 0, 0, 0], dtype=np.int64).tobytes())
            f.write(np.array(ref.LIMITS, dtype=np.float32).tobytes())
            for b in (m, rows):
                for k, dt in (("keys", np.int32), ("log_odds", np.float32), ("occ", np.uint8), ("infl", np.uint8)):
                    f.write(np.ascontiguousarray(b[k], dtype=dt).tobytes())
        subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:128], dtype=np.int64)
        nb2, pr, at = int(head[14]), int(head[15]), 128
        out = {"per_row": np.frombuffer(raw[at:at + pr * 16], dtype=np.int32).reshape(pr, 4)}
        at += pr * 16
        for k, dt, cols in (("keys", np.int32, 3), ("log_odds", np.float32, C), ("occ", np.uint8, C), ("infl", np.uint8, C)):
            size = nb2 * cols * np.dtype(dt).itemsize
            out[k] = np.frombuffer(raw[at:at + size], dtype=dt).reshape(nb2, cols)
            at += size
        assert at == len(raw)
        out.update(status=int(head[0]), code=int(head[1]), summary=head[2:14].copy())
        return out

    return run


def cube_keys(rng, count, bounds=True):
    """count distinct keys of a cube around zero — both sides of it — with a few at the key bounds"""
    side = max(2, int(np.ceil((2.5 * count) ** (1 / 3))))
    flat = rng.choice(side ** 3, count, replace=False)
    keys = (np.stack([flat % side, (flat // side) % side, flat // (side * side)], axis=1) - side // 2).astype(np.int32).reshape(count, 3)
    if bounds and count >= 2:
        k = min(len(BOUND_KEYS), count // 2)
        keys[:k] = BOUND_KEYS[:k]
    return keys[rng.permutation(count)].reshape(count, 3)


def values(rng, shape):
    """log-odds in and beyond the clamp range, with exactly occupied_sh, log_odds_min and log_odds_max among them"""
    v = rng.uniform(-3.0, 5.5, size=shape).astype(np.float32)
    pick = rng.random(shape)
    for q, x in ((0.06, SH), (0.12, LO_MIN), (0.18, LO_MAX), (0.2, np.float32(0.0))):
        v[(pick < q) & (pick >= q - 0.06)] = x
    return v


def wild(rng, keys, C):
    """a dump as anything may write it: classes and log-odds unrelated, some blank rows, some rows with only infl"""
    nb = len(keys)
    b = {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": values(rng, (nb, C)),
         "occ": rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(nb, C)), "infl": rng.choice(np.frombuffer(b"uuo", dtype=np.uint8), size=(nb, C))}
    kind = rng.random(nb)
    b["occ"][kind < 0.3] = ref.U
    b["infl"][kind < 0.15] = ref.U
    return b


def consistent(rng, keys, C):
    """a map as the merge leaves it: seen voxels inside the clamp range with occ == 'o' iff L > occupied_sh, unseen ones +0.0f / 'u'"""
    nb = len(keys)
    lo = ref.clamp(values(rng, (nb, C)), ref.LIMITS)
    seen = rng.random((nb, C)) < 0.6
    seen[rng.random(nb) < 0.2] = False
    lo[~seen] = np.float32(0.0)
    occ = np.where(seen, np.where(lo > SH, ref.O, ref.F), ref.U).astype(np.uint8)
    return {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": lo, "occ": occ,
            "infl": rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(nb, C))}


def overlapping(rng, nr, C, make=wild):
    """nr rows and a map that holds about half of their keys and as many other blocks"""
    allk = cube_keys(rng, 2 * nr + 1)
    rows = make(rng, allk[:nr], C)
    held = np.concatenate([allk[:nr][rng.random(nr) < 0.5], allk[nr:nr + 1 + nr // 2]])
    return make(rng, held[rng.permutation(len(held))], C), rows


def same(a, b, what=""):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


@pytest.mark.parametrize("n", NS)
def test_driver_equals_the_reference(driver, n):
    rng = np.random.default_rng(100 + n)
    C = n ** 3
    for nr in NROWS:
        m, rows = overlapping(rng, nr, C)
        for mode in (ref.ADD, ref.MAX, ref.TAKE, ref.FILL):
            for infl_given in (True, False):
                real = None
                for dry in (False, True):
                    what = f"n {n} rows {nr} mode {mode} infl {infl_given} dry {dry}"
                    want, sm, pr = ref.fuse(m, rows, mode, dry=dry, infl_given=infl_given)
                    got = driver(m, rows, n, mode, ref.DRY if dry else 0, infl_given, cap=len(m["keys"]))
                    assert got["status"] == ref.OK and got["code"] == 0, what
                    same(got, want, what)
                    assert got["summary"].tolist() == sm.tolist(), what
                    assert got["per_row"].tolist() == pr.tolist(), what
                    assert sm[4] == sm[5] + sm[6] + sm[7] and sm[0] == nr and sm[2] == int((pr[:, 3] == 1).sum()), what
                    if dry:  # the same counts as the real call, and every byte as it was
                        same(want, m, what)
                        assert sm.tolist() == real[0].tolist() and pr.tolist() == real[1].tolist(), what
                    else:
                        real = (sm, pr)
                        assert len(want["keys"]) == len(m["keys"]) + sm[2]
                        assert np.array_equal(want["keys"][len(m["keys"]):], rows["keys"][pr[:, 3] == 1]), what  # created slots in row order
        if nr >= 63:
            assert real[0][2] > 0 and real[0][3] > 0 and (real[1][:, 3] == 2).any()


def dense(b, union, C):
    """log-odds and classes of the blocks `union` names, 0.0f / 'u' where b holds none"""
    at = {tuple(k): i for i, k in enumerate(np.asarray(b["keys"]).tolist())}
    lo = np.zeros((len(union), C), dtype=np.float32)
    occ = np.full((len(union), C), ref.U, dtype=np.uint8)
    for r, k in enumerate(union):
        if k in at:
            lo[r], occ[r] = b["log_odds"][at[k]], b["occ"][at[k]]
    return lo, occ


@pytest.mark.parametrize("n", [2, 4])
def test_add_is_the_merge_rule_and_commutes(n):
    """on consistent maps ADD equals merge.py's finish over the key union, float bits and classes; and A into B equals B into A where
    either has seen the voxel"""
    from mlmapping_amd import mlmap

    mlmap.load_library()  # (before torch: the library then shares torch's HIP runtime process-wide, whichever test runs first)
    import torch
    from mlmapping_amd.config import S1
    from mlmapping_amd.merge import _finish_torch

    cfg = S1
    assert (np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max), np.float32(cfg.lm_occupied_sh)) == (LO_MIN, LO_MAX, SH)
    finish = _finish_torch(cfg)
    rng = np.random.default_rng(7 + n)
    C, total = n ** 3, 0
    while total < 200000:
        A, B = overlapping(rng, 300, C, make=consistent)
        union = sorted({tuple(k) for k in A["keys"].tolist()} | {tuple(k) for k in B["keys"].tolist()})
        la, oa = dense(A, union, C)
        lb, ob = dense(B, union, C)
        lo = torch.from_numpy(la + lb)
        occ = finish(lo, torch.from_numpy(((oa != ref.U) | (ob != ref.U)).astype(np.uint8))).numpy()
        ab, sm, _ = ref.fuse(A, B, ref.ADD, infl_given=False)
        ba, _, _ = ref.fuse(B, A, ref.ADD, infl_given=False)
        got_lo, got_occ = dense(ab, union, C)
        assert got_lo.tobytes() == lo.numpy().tobytes() and got_occ.tobytes() == occ.tobytes()
        rev_lo, rev_occ = dense(ba, union, C)
        seen = got_occ != ref.U
        assert np.array_equal(seen, rev_occ != ref.U)
        assert np.array_equal(got_lo.view(np.uint32)[seen], rev_lo.view(np.uint32)[seen]) and np.array_equal(got_occ[seen], rev_occ[seen])
        assert sm[4] == sm[5] + sm[6] + sm[7] and sm[7] > 0 and sm[5] > 0
        total += len(union) * C


@pytest.mark.parametrize("n", [2, 3])
def test_properties_of_the_rule(driver, n):
    rng = np.random.default_rng(50 + n)
    C = n ** 3
    # MAX, TAKE and FILL of a map into itself change nothing
    A = consistent(rng, cube_keys(rng, 257), C)
    for mode in (ref.MAX, ref.TAKE, ref.FILL):
        after, sm, pr = ref.fuse(A, A, mode)
        same(after, A, f"self mode {mode}")
        assert sm[11] == 0 and sm[8] == sm[9] == sm[10] == sm[2] == sm[7] == 0 and not pr[:, 1:].any()
        got = driver(A, A, n, mode)
        same(got, A, f"driver self mode {mode}")
        assert got["summary"].tolist() == sm.tolist()
    # FILL never changes a seen voxel, whatever the input; an incoming NaN or infinity gives a finite result
    m, rows = overlapping(rng, 257, C)
    rows["log_odds"][rng.random(rows["log_odds"].shape) < 0.2] = np.nan
    rows["log_odds"][rng.random(rows["log_odds"].shape) < 0.1] = np.inf
    rows["log_odds"][rng.random(rows["log_odds"].shape) < 0.1] = -np.inf
    for mode in (ref.ADD, ref.MAX, ref.TAKE, ref.FILL):
        after, sm, pr = ref.fuse(m, rows, mode)
        nb = len(m["keys"])
        assert np.isfinite(after["log_odds"]).all() and sm[4] == sm[5] + sm[6] + sm[7]
        written = after["log_odds"].view(np.uint32)[:nb] != m["log_odds"].view(np.uint32)
        assert (after["log_odds"][:nb][written] >= LO_MIN).all() and (after["log_odds"][:nb][written] <= LO_MAX).all()
        if mode == ref.FILL:
            seen = m["occ"] != ref.U
            assert np.array_equal(after["log_odds"].view(np.uint32)[:nb][seen], m["log_odds"].view(np.uint32)[seen])
            assert np.array_equal(after["occ"][:nb][seen], m["occ"][seen]) and sm[9] == 0
        got = driver(m, rows, n, mode)
        same(got, after, f"driver wild mode {mode}")
        assert got["summary"].tolist() == sm.tolist() and got["per_row"].tolist() == pr.tolist()
    # a dump with no contributing voxel and no infl creates no block — and with infl given it does
    blank = wild(rng, cube_keys(rng, 65), C)
    blank["occ"][:] = ref.U
    empty = {"keys": np.zeros((0, 3), np.int32), "log_odds": np.zeros((0, C), np.float32), "occ": np.zeros((0, C), np.uint8), "infl": np.zeros((0, C), np.uint8)}
    after, sm, pr = ref.fuse(empty, blank, ref.TAKE, infl_given=False)
    assert len(after["keys"]) == 0 and sm[2] == 0 and sm[3] == 65 and (pr[:, 3] == 2).all() and not sm[4:].any()
    got = driver(empty, blank, n, ref.TAKE, infl_given=False)
    assert len(got["keys"]) == 0 and got["summary"].tolist() == sm.tolist()
    after, sm, pr = ref.fuse(empty, blank, ref.TAKE, infl_given=True)
    assert sm[2] == int((blank["infl"] == ref.O).any(axis=1).sum()) > 0 and sm[10] == int((blank["infl"] == ref.O).sum()) and sm[11] == 0
    same(driver(empty, blank, n, ref.TAKE), after, "infl only")


def test_model_pool_growth_and_capacity(driver):
    """the created blocks beyond the model pool: refused untouched when it may not grow, grown before the first write when it may"""
    rng = np.random.default_rng(5)
    n, C = 2, 8
    m, rows = overlapping(rng, 65, C)
    want, sm, pr = ref.fuse(m, rows, ref.ADD)
    assert sm[2] > 3
    got = driver(m, rows, n, cap=len(m["keys"]) + int(sm[2]) - 1, grow=False)
    assert got["status"] == ref.ERR_CAPACITY and not got["summary"].any()
    same(got, m, "refused")
    for cap in (len(m["keys"]) + int(sm[2]), len(m["keys"]) + int(sm[2]) - 1):
        got = driver(m, rows, n, cap=cap, grow=cap < len(m["keys"]) + int(sm[2]))
        assert got["status"] == ref.OK
        same(got, want, f"cap {cap}")
    got = driver(m, rows, n, flags=ref.DRY, cap=len(m["keys"]), grow=False)  # a diff needs no room
    assert got["status"] == ref.OK and got["summary"].tolist() == sm.tolist()


INVALID = [(dict(rows_n=-1), 1), (dict(rows_n=-(1 << 31)), 1),
           (dict(null=("keys",)), 2), (dict(null=("log_odds",)), 2), (dict(null=("occ",)), 2), (dict(null=("keys", "occ")), 2),
           (dict(mode=4), 3), (dict(mode=-1), 3), (dict(mode=1 << 20), 3),
           (dict(flags=2), 4), (dict(flags=3), 4), (dict(flags=-1), 4), (dict(flags=1 << 30), 4)]
VALID = [dict(), dict(mode=3, flags=1), dict(rows_n=0, null=("keys", "log_odds", "occ")), dict(infl_given=False), dict(mode=2, per_row=False)]


def test_argument_check(driver):
    rng = np.random.default_rng(1)
    m, rows = overlapping(rng, 2, 8)
    none = {k: v[:0] for k, v in rows.items()}
    for case, code in INVALID + [(c, 0) for c in VALID]:
        a = dict(mode=ref.ADD, flags=0, infl_given=True, per_row=True, rows_n=None, null=())
        a.update(case)
        r = rows if a["rows_n"] is None else none
        nr = len(r["keys"]) if a["rows_n"] is None else a["rows_n"]
        present = lambda k: None if k in a["null"] else r[k]
        assert ref.check_args(nr, present("keys"), present("log_odds"), present("occ"), a["mode"], a["flags"]) == code, case
        got = driver(m, r, 2, **a)
        assert got["code"] == code and got["status"] == (ref.ERR_INVALID if code else ref.OK), (case, got["code"])
        if code or nr == 0:
            assert not got["summary"].any() and len(got["per_row"]) == 0
            same(got, m, str(case))


def test_bad_keys_leave_the_map_untouched(driver):
    rng = np.random.default_rng(2)
    n, C = 3, 27
    m, rows = overlapping(rng, 65, C)
    for mode in (ref.ADD, ref.FILL):
        for flags in (0, ref.DRY):
            for which, code in (("dup", 6), ("range", 5), ("both", 5)):
                bad = {k: v.copy() for k, v in rows.items()}
                if which in ("dup", "both"):
                    bad["keys"][40] = bad["keys"][3]
                if which in ("range", "both"):
                    bad["keys"][64] = [0, ref.KEY_MAX + 1, 0] if mode == ref.ADD else [ref.KEY_MIN - 1, 0, 0]
                assert ref.check_keys(bad["keys"]) == code
                got = driver(m, bad, n, mode, flags)
                assert got["status"] == ref.ERR_INVALID and got["code"] == code and not got["summary"].any() and len(got["per_row"]) == 0
                same(got, m, f"{which} mode {mode} flags {flags}")
    assert ref.check_keys(rows["keys"]) == 0 and ref.check_keys(np.array([[ref.KEY_MAX, ref.KEY_MIN, 0]])) == 0
    # keys that differ only beyond the packed 21 bits are out of range, not duplicates of each other
    assert ref.check_keys(np.array([[0, 0, 0], [1 << 21, 0, 0]])) == 5


def test_binding_names_the_call():
    from mlmapping_amd import mlmap

    assert "mlm_fuse_blocks" in mlmap.ABI_SYMBOLS
    assert (mlmap.MLM_FUSE_ADD, mlmap.MLM_FUSE_MAX, mlmap.MLM_FUSE_TAKE, mlmap.MLM_FUSE_FILL) == (ref.ADD, ref.MAX, ref.TAKE, ref.FILL)
    assert (mlmap.MLM_FUSE_DRY, mlmap.MLM_FUSE_ROW, mlmap.MLM_FUSE_COLS) == (ref.DRY, ref.ROW, ref.COLS) and mlmap.FUSE_MODES == ref.MODES
    assert hasattr(mlmap.MLMap, "fuse_blocks") and hasattr(mlmap.MLMap, "fuse_from")
    header = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    assert "int mlm_fuse_blocks(mlm_handle *h, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ," in header
    assert "enum { MLM_FUSE_ADD = 0, MLM_FUSE_MAX = 1, MLM_FUSE_TAKE = 2, MLM_FUSE_FILL = 3 };" in header and "#define MLM_FUSE_ROW 12" in header
    assert header.index("int mlm_warp_blocks(") < header.index("int mlm_fuse_blocks(") < header.index("int mlm_merge_pack(")
    assert "mlm_fuse_blocks(h_, n, keys, log_odds, occ, infl, mode, flags, per_row, summary)" in open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
    fuse_h = open(os.path.join(CSRC, "mlm_fuse.h")).read()
    for name, v in (("M_ADD", 0), ("M_MAX", 1), ("M_TAKE", 2), ("M_FILL", 3), ("F_DRY", 1), ("SUMS", 12), ("PR", 4)):
        assert f"#define MLM_FUSE_{name} {v}" in fuse_h


def test_facade_member_compiles(tmp_path):
    """include/mlmap_facade.hpp's fuseBlocks as a C++ client calls it (tests/cpp/fuse_client.cpp)"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "fuse_client.cpp"),
                           "-o", str(tmp_path / "fuse_client.o")])
