"""Ground truth of mlm_query_boxes (include/mlmap_hip.h) for tests/test_box_grow.py and tests/test_gpu_boxes.py: the contract's
validity rules, limits, rounds and faces written in plain Python integers over a class function (raywalk_ref.block_classes of a
block dump, or any other callable voxels [K,3] -> MLM_BOX_* bits), and the property checks the growth is held to.  Nothing here
calls the code under test."""
import numpy as np

from tests import raywalk_ref as rw

OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN
FLAG_SETS = (0, 1, 2, 4, 3, 5, 7)
OUTPUTS = ("status", "box", "closed", "table")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
MAX_SIDE = 2 ** 15


def grow_limits(max_grow):
    """the six layer counts: None is all zero, one int stands for all six faces"""
    if max_grow is None:
        return [0] * 6
    return [int(max_grow)] * 6 if np.ndim(max_grow) == 0 else [int(v) for v in max_grow]


def box_voxels(lo, hi):
    """the voxels of the inclusive box lo .. hi as [K,3] int64"""
    ax = [np.arange(int(lo[a]), int(hi[a]) + 1, dtype=np.int64) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def window_limits(window):
    """(first voxel, last voxel) per axis of a window (lo, dims), or None"""
    if window is None:
        return None
    lo, dims = [int(v) for v in window[0]], [int(v) for v in window[1]]
    return lo, [lo[a] + dims[a] - 1 for a in range(3)]


def valid(b6, W):
    a, b = [int(v) for v in b6[:3]], [int(v) for v in b6[3:]]
    for k in range(3):
        if a[k] > b[k] or b[k] - a[k] >= MAX_SIDE:
            return False
        if W is not None and (a[k] < W[0][k] or b[k] > W[1][k]):
            return False
    return True


def at_limit(lo, hi, c, grown, max_grow, W):
    """the next layer of face c, and whether taking it would pass a limit"""
    ax, up = c >> 1, c & 1
    nxt = hi[ax] + 1 if up else lo[ax] - 1
    lim = grown[c] >= max_grow[c] or nxt > I32_MAX or nxt < I32_MIN or (W is not None and (nxt < W[0][ax] or nxt > W[1][ax]))
    return nxt, lim


def slab(lo, hi, c, nxt):
    slo, shi = list(lo), list(hi)
    slo[c >> 1] = shi[c >> 1] = nxt
    return slo, shi


def grow(b6, flags, classes, max_grow=None, window=None):
    """(status, out6, closed, row) of one item"""
    W = window_limits(window)
    mg = grow_limits(max_grow)
    b6 = [int(v) for v in b6]
    if not valid(b6, W):
        return -1, tuple(b6), 0, (0, 0, 0, 0)
    lo, hi = b6[:3], b6[3:]
    bits = classes(box_voxels(lo, hi))
    unk = int(((bits & UNKNOWN) != 0).sum())
    obs = int(((bits & flags) != 0).sum())
    if obs:
        return 0, tuple(b6), 0, (len(bits), unk, obs, 0)
    grown = [0] * 6
    is_open = [True] * 6
    closed = 0
    slabs = 0
    while any(is_open):
        for c in range(6):
            if not is_open[c]:
                continue
            nxt, lim = at_limit(lo, hi, c, grown, mg, W)
            if lim:
                is_open[c] = False
                continue
            sb = classes(box_voxels(*slab(lo, hi, c, nxt)))
            if ((sb & flags) != 0).any():
                is_open[c] = False
                closed |= 1 << c
                continue
            if c & 1:
                hi[c >> 1] = nxt
            else:
                lo[c >> 1] = nxt
            grown[c] += 1
            unk += int(((sb & UNKNOWN) != 0).sum())
            slabs += 1
    vol = (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1)
    return 1, tuple(lo + hi), closed, (vol, unk, 0, slabs)


def grow_all(boxes, flags, classes, max_grow=None, window=None):
    """{"status", "box", "closed", "table"} as arrays with mlm_query_boxes' types"""
    boxes = np.asarray(boxes).reshape(-1, 6)
    n = len(boxes)
    out = {"status": np.empty(n, np.int8), "box": np.empty((n, 6), np.int32), "closed": np.empty(n, np.uint8), "table": np.empty((n, 4), np.int64)}
    for i in range(n):
        out["status"][i], out["box"][i], out["closed"][i], out["table"][i] = grow(boxes[i], flags, classes, max_grow, window)
    return out


def assert_equal(got, exp, what=""):
    for k in OUTPUTS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, g.dtype, e.shape, e.dtype)
        bad = np.flatnonzero((g != e).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what} {k}: {bad.size} of {len(g)} boxes differ, first #{bad[0]}: {g[bad[0]]!r} vs {e[bad[0]]!r}"


def check_properties(b6, flags, classes, max_grow, window, res):
    """what makes a grown box right, independent of the order of the rounds: B0 inside the result, no O voxel in it, inside the limits,
    an O voxel in the adjacent slab of every face closed by obstacle, every other face exactly at a limit (maximality), and the
    counts.  Returns the status."""
    status, out6, closed, row = res
    W = window_limits(window)
    mg = grow_limits(max_grow)
    b6 = [int(v) for v in b6]
    if not valid(b6, W):
        assert res == (-1, tuple(b6), 0, (0, 0, 0, 0))
        return -1
    a, b = b6[:3], b6[3:]
    bits0 = classes(box_voxels(a, b))
    if ((bits0 & flags) != 0).any():
        assert status == 0 and out6 == tuple(b6) and closed == 0
        assert row == (len(bits0), int(((bits0 & UNKNOWN) != 0).sum()), int(((bits0 & flags) != 0).sum()), 0)
        return 0
    assert status == 1
    lo, hi = list(out6[:3]), list(out6[3:])
    grown = []
    for k in range(3):
        assert lo[k] <= a[k] and b[k] <= hi[k]  # B0 inside the result
        grown += [a[k] - lo[k], hi[k] - b[k]]
        assert grown[-2] <= mg[2 * k] and grown[-1] <= mg[2 * k + 1]  # within max_grow ...
        assert I32_MIN <= lo[k] and hi[k] <= I32_MAX
        if W is not None:
            assert W[0][k] <= lo[k] and hi[k] <= W[1][k]  # ... and within the window
    bits = classes(box_voxels(lo, hi))
    assert not ((bits & flags) != 0).any()  # no O voxel
    assert row == (len(bits), int(((bits & UNKNOWN) != 0).sum()), 0, sum(grown))
    for c in range(6):
        nxt, lim = at_limit(lo, hi, c, grown, mg, W)
        if closed >> c & 1:
            assert not lim
            sb = classes(box_voxels(*slab(lo, hi, c, nxt)))
            assert ((sb & flags) != 0).any(), ("face closed by obstacle without one in its slab", c)
        else:
            assert lim, ("face closed by limit away from every limit", c)
    assert closed < 64
    return 1
