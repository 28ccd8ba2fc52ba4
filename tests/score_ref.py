"""Ground truth of mlm_score_poses (include/mlmap_hip.h) for tests/test_score_plan.py and tests/test_gpu_score.py: the contract in
numpy float64 and int64, every floating-point step an explicit elementwise operation in the contract's order (no matmul, no einsum:
they may fuse or reorder), over voxel classes taken from a block dump (raywalk_ref.block_classes) or any other callable.  Nothing
here calls the code under test."""
import numpy as np

from tests import raywalk_ref as rw

ROW = 8
WORDS = ("valid", "occ", "free", "unknown", "infl", "in_box", "cost", "zero")
OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN


def world(pts_s, T_ws):
    """w[k, j, a] = ((R[a][0] * s0 + R[a][1] * s1) + R[a][2] * s2) + o[a] of point j under pose k"""
    s = np.asarray(pts_s, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T_ws, dtype=np.float64).reshape(-1, 12)
    w = np.empty((len(T), len(s), 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for a in range(3):
            t = T[:, 3 * a, None] * s[None, :, 0]
            u = T[:, 3 * a + 1, None] * s[None, :, 1]
            t = t + u
            u = T[:, 3 * a + 2, None] * s[None, :, 2]
            t = t + u
            w[:, :, a] = t + T[:, 9 + a, None]
    return w


def voxels(w, d):
    """(valid [k, j], v [k, j, 3] int64): Q = floor((w / d) * 1024.0), valid if every Q is finite and |Q| < 2^40, v = Q >> 10"""
    with np.errstate(all="ignore"):
        q = w / np.float64(d)
        q = q * 1024.0
        q = np.floor(q)
        valid = (np.isfinite(q) & (np.abs(q) < 2.0 ** 40)).all(axis=-1)
    Q = np.where(valid[..., None], q, 0.0).astype(np.int64)
    return valid, Q >> 10


def score(pts_s, T_ws, d, classes=None, box=None, sqdist=None, sq_cap=64):
    """table int64 [n_poses][8]; classes: a callable voxels [K, 3] -> MLM_RAY_* bits, or None; box = (lo, dims) with sqdist
    [dims2][dims1][dims0] int32, or None"""
    valid, v = voxels(world(pts_s, T_ws), d)
    n = valid.shape[0]
    table = np.zeros((n, ROW), dtype=np.int64)
    table[:, 0] = valid.sum(axis=1)
    if classes is not None:
        for k in range(n):  # (pose by pose: the class lookup sorts its voxels)
            bits = classes(v[k][valid[k]])
            table[k, 1] = ((bits & OCC) != 0).sum()
            table[k, 2] = ((bits & (OCC | UNKNOWN)) == 0).sum()
            table[k, 3] = ((bits & UNKNOWN) != 0).sum()
            table[k, 4] = ((bits & INFL) != 0).sum()
    if box is not None:
        lo, dims = (np.asarray(x, dtype=np.int64).reshape(3) for x in box)
        f = np.asarray(sqdist, dtype=np.int32).reshape(-1).astype(np.int64)
        assert f.size == dims.prod()
        r = v - lo
        inside = valid & ((r >= 0) & (r < dims)).all(axis=-1)
        at = np.where(inside, (r[..., 2] * dims[1] + r[..., 1]) * dims[0] + r[..., 0], 0)
        sq = f[at]
        cost = np.where(inside, np.minimum(np.maximum(sq, 0), sq_cap), sq_cap)
        table[:, 5] = inside.sum(axis=1)
        table[:, 6] = np.where(valid, cost, 0).sum(axis=1)
        table[:, 7] = (inside & (sq <= 0)).sum(axis=1)
    return table


def best_row(table):
    """the smallest [6], ties to the largest [1], then to the lowest index"""
    t = np.asarray(table, dtype=np.int64)
    key = [(int(t[k, 6]), -int(t[k, 1]), k) for k in range(len(t))]
    return min(key)[2]


def assert_equal(got, exp, what=""):
    """every word of every row equal; names the first pose and word that differ"""
    g, e = np.asarray(got), np.asarray(exp)
    assert g.dtype == np.int64 and g.shape == e.shape, (what, g.dtype, g.shape, e.shape)
    bad = np.argwhere(g != e)
    if len(bad):
        k, w = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} words of {len(np.unique(bad[:, 0]))} poses differ, first pose #{k} word [{w}] "
                             f"({WORDS[w]}): {int(g[k, w])} vs {int(e[k, w])}; row {g[k].tolist()} vs {e[k].tolist()}")


def non_vacuous(table, what=""):
    """the conditions that keep a comparison from passing vacuously, on a reference table computed with classes and a field"""
    t = np.asarray(table, dtype=np.int64)
    tot = t.sum(axis=0)
    assert all(tot[w] >= 50 for w in (1, 2, 3, 4)), (what, tot.tolist())
    assert tot[0] <= 4 * tot[5] and 4 * tot[5] <= 3 * tot[0], (what, tot.tolist())
    assert 2 * len(np.unique(t, axis=0)) >= len(t), (what, len(np.unique(t, axis=0)), len(t))
    return tot


def random_rotations(rng, count):
    """count x 9 row-major rotation matrices from normalised random quaternions"""
    q = rng.normal(size=(count, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)


IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
