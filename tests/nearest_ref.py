"""Ground truth of mlm_query_nearest (include/mlmap_hip.h) for tests/test_nearest_plan.py and tests/test_gpu_nearest.py: the contract
written in plain Python integers — every voxel of the cube v +- C is enumerated, no pruning, and the answer is the minimum of
(E, z, y, x) tuples, independent of the packed key — over voxel classes taken from a block dump (raywalk_ref.block_classes) or from
any other callable.  Nothing here calls the code under test."""
import math

import numpy as np

from tests import raywalk_ref as rw

OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN
FLAG_SETS = tuple(f for f in rw.FLAG_SETS if f)
OUTPUTS = ("status", "voxel", "delta", "sq", "dist")
NONE = -1

_offsets = {}


def cube_offsets(C):
    """the (2C + 1)^3 offsets of the cube as an int64 array, z slowest (any order would do)"""
    if C not in _offsets:
        r = np.arange(-C, C + 1, dtype=np.int64)
        z, y, x = np.meshgrid(r, r, r, indexing="ij")
        _offsets[C] = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return _offsets[C]


def dist_of(sq, d):
    """the three double operations of the contract: (double)(float)subbox_d_xyz * sqrt((double)E) / 1024.0"""
    return (float(np.float32(d)) * math.sqrt(float(sq))) / 1024.0  # (sq < 2^53: exact as a double; math.sqrt is correctly rounded)


def candidates(Q, C, classes, flags):
    """the point's voxel, the (E, z, y, x) tuples of the two smallest candidates — voxels of the cube with O inside the ball — in
    order, and whether the cube holds a voxel with O outside the ball"""
    v = [q >> 10 for q in Q]
    vox = cube_offsets(C) + np.array(v, dtype=np.int64)
    vox = vox[(classes(vox) & flags) != 0]
    dl = 1024 * vox + 512 - np.array(Q, dtype=np.int64)  # (|Q| < 2^40 and |delta| < 2^17: nothing leaves int64)
    E = (dl * dl).sum(axis=1)
    ball = E <= (1024 * C) ** 2
    E, inside = E[ball], vox[ball]
    first = np.lexsort((inside[:, 0], inside[:, 1], inside[:, 2], E))[:2]  # (the last key is the primary one)
    return v, [(int(E[i]), int(inside[i, 2]), int(inside[i, 1]), int(inside[i, 0])) for i in first], bool((~ball).any())


def nearest(pos, d, C, classes, flags):
    """(status, voxel, delta, sq, dist) of one position, and what decided it: {"tie": None or the axis (2 z, 1 y, 0 x) on which the
    winner beat the runner-up at equal E, "cube_differs": a rule that took the nearest voxel of the cube v +- C would answer, the
    ball rule does not}"""
    Q = rw.lattice(pos, d)
    if Q is None:
        return (-1, (0, 0, 0), (0, 0, 0), NONE, -1.0), {"tie": None, "cube_differs": False}
    v, inside, outside = candidates(Q, C, classes, flags)
    if not inside:
        return (0, tuple(v), (0, 0, 0), NONE, -1.0), {"tie": None, "cube_differs": outside}
    E, z, y, x = min(inside)  # (tuples compare as the contract's rule reads: E, then z, then y, then x)
    tie = None
    if len(inside) > 1 and max(inside)[0] == E:
        other = max(inside)
        tie = 2 if other[1] != z else (1 if other[2] != y else 0)
    o = (x, y, z)
    delta = tuple(1024 * o[a] + 512 - Q[a] for a in range(3))
    return (1, o, delta, E, dist_of(E, d)), {"tie": tie, "cube_differs": False}


def nearest_all(pos, d, C, classes, flags):
    """{"status", "voxel", "delta", "sq", "dist"} as arrays with mlm_query_nearest's types, and the list of what decided each"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    res = {"status": np.empty(n, np.int8), "voxel": np.empty((n, 3), np.int32), "delta": np.empty((n, 3), np.int32),
           "sq": np.empty(n, np.int64), "dist": np.empty(n, np.float64)}
    why = []
    for i in range(n):
        r, w = nearest(pos[i], d, C, classes, flags)
        res["status"][i], res["voxel"][i], res["delta"][i], res["sq"][i], res["dist"][i] = r
        why.append(w)
    return res, why


def assert_equal(got, exp, what=""):
    """every output present equal: integers exactly, dist by its 64 bits"""
    for k in OUTPUTS:
        if k not in got:
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, g.dtype, e.shape, e.dtype)
        bad = (g.view(np.uint64) != e.view(np.uint64)) if k == "dist" else (g != e)
        bad = np.flatnonzero(bad.reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what} {k}: {bad.size} of {len(g)} points differ, first #{bad[0]}: {g[bad[0]]!r} vs {e[bad[0]]!r}"


def check_properties(pos, d, C, classes, flags, res):
    """the answer satisfies O, lies in the ball, and no voxel of the cube with O inside the ball has a smaller tuple; without an
    answer no voxel of the cube has O inside the ball — checked voxel by voxel, without sorting"""
    status, o, delta, sq, dist = res
    Q = rw.lattice(pos, d)
    if Q is None:
        assert res == (-1, (0, 0, 0), (0, 0, 0), NONE, -1.0)
        return -1
    v = [q >> 10 for q in Q]
    vox = cube_offsets(C) + np.array(v, dtype=np.int64)
    has = (classes(vox) & flags) != 0
    dl = 1024 * vox + 512 - np.array(Q, dtype=np.int64)
    E = (dl * dl).sum(axis=1)
    ball = E <= (1024 * C) ** 2
    if status == 0:
        assert not (has & ball).any() and o == tuple(v) and delta == (0, 0, 0) and sq == NONE and dist == -1.0
        return 0
    assert status == 1
    assert int(classes(np.array([o]))[0]) & flags, "the answer has no O"
    assert sq == sum(x * x for x in delta) and sq <= (1024 * C) ** 2 and all(delta[a] == 1024 * o[a] + 512 - Q[a] for a in range(3))
    assert all(abs(o[a] - v[a]) <= C for a in range(3))
    cand = has & ball
    smaller = cand & ((E < sq) | ((E == sq) & ((vox[:, 2] < o[2]) | ((vox[:, 2] == o[2]) & ((vox[:, 1] < o[1]) | ((vox[:, 1] == o[1]) & (vox[:, 0] < o[0])))))))
    assert not smaller.any(), "a voxel of the cube has a smaller tuple"
    assert dist == dist_of(sq, d)
    return 1
