"""Ground truth of mlm_query_clearance (include/mlmap_hip.h) for tests/test_clearance_plan.py and tests/test_gpu_clearance.py: the
contract written in plain Python integers on tests/raywalk_ref.py's path — every path voxel looked up on its own from its absolute
index, no incremental index, no look-ahead.  Nothing here calls the code under test."""
import numpy as np

from tests import raywalk_ref as rw

OUTSIDE_PASS, NONE, LEFT, ROW = 1, -1, 2, 8
OUTPUTS = ("status", "voxel", "t", "n_steps", "min_sq", "min", "cost", "n_near")
TYPES = {"status": (np.int8, ()), "voxel": (np.int32, (3,)), "t": (np.float64, ()), "n_steps": (np.int32, ()), "min_sq": (np.int32, ()),
         "min": (np.int32, (3,)), "cost": (np.int64, ()), "n_near": (np.int32, ())}


def field_at(v, lo, dims, sqdist, sq_cap):
    """f(v) for v in the box, None outside; sqdist is [dz][dy][dx]"""
    r = [int(v[a]) - int(lo[a]) for a in range(3)]
    if any(r[a] < 0 or r[a] >= int(dims[a]) for a in range(3)):
        return None
    return min(max(int(sqdist[r[2], r[1], r[0]]), 0), int(sq_cap))


def walk(p0, p1, d, lo, dims, sqdist, sq_stop, sq_cap, outside_pass):
    """(status, voxel, t, n_steps, min_sq, min3, cost, n_near) of one segment"""
    Q = rw.valid(p0, p1, d)
    if Q is None:
        return -1, (0, 0, 0), 0.0, 0, NONE, (0, 0, 0), 0, 0
    pth, _ = rw.path(*Q)
    seen = []  # (f, voxel)
    passed = 0
    for k, (v, (m, ad)) in enumerate(pth):
        f = field_at(v, lo, dims, sqdist, sq_cap)
        if f is None:
            if not outside_pass:
                return _result(LEFT, v, m / ad, k, seen, passed, sq_cap)
            f = int(sq_cap)
        if f <= sq_stop:
            return _result(1, v, m / ad, k, seen + [(f, v)], passed, sq_cap)
        seen.append((f, v))
        passed += 1
    return _result(0, pth[-1][0], 1.0, len(pth), seen, passed, sq_cap)


def _result(status, v, t, k, seen, passed, sq_cap):
    assert passed == k
    if seen:
        mn = min(f for f, _ in seen)
        mv = next(u for f, u in seen if f == mn)
    else:
        mn, mv = NONE, (0, 0, 0)
    cost = sum(int(sq_cap) - f for f, _ in seen[:passed])
    near = sum(1 for f, _ in seen[:passed] if f < sq_cap)
    return status, tuple(v), t, k, mn, tuple(mv), cost, near


def clearance_all(p0, p1, d, lo, dims, sqdist, sq_stop, sq_cap, outside_pass=False):
    """the eight outputs as arrays with mlm_query_clearance's types"""
    p0, p1 = np.asarray(p0, dtype=np.float64).reshape(-1, 3), np.asarray(p1, dtype=np.float64).reshape(-1, 3)
    n = len(p0)
    sq = np.asarray(sqdist).reshape(int(dims[2]), int(dims[1]), int(dims[0]))
    res = {k: np.empty((n,) + TYPES[k][1], dtype=TYPES[k][0]) for k in OUTPUTS}
    for i in range(n):
        o = walk(p0[i], p1[i], d, lo, dims, sq, sq_stop, sq_cap, outside_pass)
        for k, val in zip(OUTPUTS, o):
            res[k][i] = val
    return res


def group_rows(res, group_begin):
    """table int64 [n_groups][8] from the per-ray answers"""
    gb = [int(x) for x in group_begin]
    table = np.empty((len(gb) - 1, ROW), dtype=np.int64)
    for g in range(len(gb) - 1):
        b, e = gb[g], gb[g + 1]
        stop = next((i for i in range(b, e) if res["status"][i] != 0), None)
        C = range(b, e if stop is None else stop + 1)
        mins = [(int(res["min_sq"][i]), i - b) for i in C if res["min_sq"][i] != NONE]
        mn = min((m for m, _ in mins), default=-1)
        at = next((j for m, j in mins if m == mn), -1)
        table[g] = [e - b, -1 if stop is None else stop - b, 0 if stop is None else int(res["status"][stop]), mn, at,
                    sum(int(res["cost"][i]) for i in C), sum(int(res["n_steps"][i]) for i in C), sum(int(res["n_near"][i]) for i in C)]
    return table


def assert_equal(got, exp, what=""):
    """every output that is present equal byte for byte (t by its 64 bits), the table too"""
    for k in OUTPUTS + ("table",):
        if k not in got:
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, g.dtype, e.shape, e.dtype)
        if g.tobytes() == e.tobytes():
            continue
        bad = np.flatnonzero((g.reshape(len(g), -1) != e.reshape(len(e), -1)).any(axis=1))
        first = bad[0] if bad.size else 0
        raise AssertionError(f"{what} {k}: {bad.size} of {len(g)} rows differ, first #{first}: {g[first]!r} vs {e[first]!r}")


# ---- fields and segments ----------------------------------------------------------------------------------------------------------
def wild_field(rng, dims):
    """arbitrary int32 content: half of it in the range a cap of 64 does not clamp, negatives, INT32_MIN and INT32_MAX among the rest"""
    shape = (int(dims[2]), int(dims[1]), int(dims[0]))
    f = rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64).astype(np.int32)
    small = rng.random(shape) < 0.7
    f[small] = rng.integers(-3, 70, size=int(small.sum()))
    flat = f.reshape(-1)
    special = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0, -1]
    flat[rng.choice(flat.size, min(4, flat.size), replace=False)] = special[:min(4, flat.size)]
    return f


def segments(rng, lo, dims, d, count):
    """end points around the box lo, dims (voxels): both inside, one or both outside (by up to 4 voxels), zero-length ones, exact
    voxel-corner and edge crossings (rw.special_rays) and the invalid ones (rw.weird_rays)"""
    lo, dims = np.asarray(lo, dtype=np.float64), np.asarray(dims, dtype=np.float64)
    a, b = rng.uniform(lo * d, (lo + dims) * d, size=(count, 3)), rng.uniform(lo * d, (lo + dims) * d, size=(count, 3))
    out = rng.random(count)
    a[out < 0.25] = rng.uniform((lo - 4) * d, (lo + dims + 4) * d, size=(int((out < 0.25).sum()), 3))
    b[out > 0.7] = rng.uniform((lo - 4) * d, (lo + dims + 4) * d, size=(int((out > 0.7).sum()), 3))
    z = rng.random(count) < 0.05
    b[z] = a[z]
    s0, s1 = rw.special_rays(rng, float(((lo - 2) * d).min()), float(((lo + dims + 2) * d).max()), d, count=max(4, count // 16))
    w0, w1 = rw.weird_rays(d)
    return np.ascontiguousarray(np.concatenate([a, s0, w0])), np.ascontiguousarray(np.concatenate([b, s1, w1]))
