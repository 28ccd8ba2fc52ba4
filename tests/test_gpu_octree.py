"""mlm_export_octree: the exact pruned occupancy octree of a voxel box (include/mlmap_hip.h), checked byte for byte against the numpy /
Python ground truth (tests/octree_ref.py) on this library's own export_window {occ, infl} of the same box: words, inner4, skip, leaf4,
leaf_class and the summary; and the decoded word stream against the window directly.

The maps: scene S1 after four frames (subbox_n 10), maps built cell by cell through import_blocks at subbox_n 2, 3 and 16 (a brick of
16^3 voxels then spans up to 9^3 / 7^3 / 2^3 map blocks), and a frontier-mode map whose released blocks answer from element 0."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import octree_ref as ref
from tests.test_octree_plan import BOXES, FLAGS, KEYS, SENT, smallest_depth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def MLMap():
    from mlmapping_amd.mlmap import MLMap as M

    return M


def kw(flags):
    return dict(infl=bool(flags & ref.INFL), occ_only=bool(flags & ref.OCC_ONLY))


def expected(gpu, lo, dims, depth, flags):
    win = gpu.export_window(lo, dims, odds=False, occ=True, infl=True)
    exp = ref.tree(win["occ"], win["infl"], lo, depth, flags)
    ref.check(exp, depth, lo, dims)
    return exp


def same(got, exp, what=""):
    assert np.array_equal(got["summary"], exp["summary"]), (what, got["summary"], exp["summary"])
    for k, _, _, _ in KEYS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def check(gpu, lo, dims, depth, flags, what=""):
    exp = expected(gpu, lo, dims, depth, flags)
    got = gpu.export_octree(lo, dims, depth, **kw(flags))
    what = f"{what} lo={lo} dims={dims} depth={depth} flags={flags}"
    same(got, exp, what)
    # the decoded stream against the window directly
    assert np.array_equal(ref.decode(got["words"], depth, lo, dims, int(got["summary"][6])), exp["labels"]), what
    return got


def raw(gpu, lo, dims, depth, flags, arrays, cap_n, cap_m, summary=True):
    """mlm_export_octree itself: arrays {name: numpy array or device pointer}, the others NULL; returns (status, summary)"""
    from mlmapping_amd.mlmap import _p

    lo_a, dims_a = np.asarray(lo, dtype=np.int32), np.asarray(dims, dtype=np.int32)
    ptr = []
    for k, _, _, _ in KEYS:
        a = arrays.get(k)
        ptr.append(None if a is None else ctypes.c_void_p(a) if isinstance(a, int) else _p(a))
    sm = np.zeros(ref.ROW, dtype=np.int64)
    rc = gpu._L.mlm_export_octree(gpu._h, _p(lo_a), _p(dims_a), depth, flags, ptr[0], ptr[1], ptr[2], cap_n, ptr[3], ptr[4], cap_m, _p(sm) if summary else None)
    return rc, sm


# ---- scene S1 -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(MLMap):
    gpu = MLMap(S1, max_blocks=16384)
    t = None
    for img, (q, t) in syn.stream(S1, "room_jitter", "smooth", 4):
        gpu.update_map(img, q, t)
    gpu.inflate_map(t)
    b = gpu.export_blocks()
    blk, cell = np.nonzero(b["occ"] == ord("o"))
    n, pick = S1.subbox_n, len(blk) // 2
    c = int(cell[pick])
    centre = b["keys"][blk[pick]].astype(np.int64) * n + [c % n, c // n % n, c // (n * n)]
    yield gpu, [int(v) for v in centre]
    gpu.close()


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(map(str, b[0])))
def test_scene_small_boxes(scene, box):
    """the boxes of the CPU test, once where they are and once moved to an occupied voxel of the scene"""
    gpu, centre = scene
    dims, lo = box
    assert S1.subbox_n == 10
    for at in (list(lo), [centre[a] - dims[a] // 2 for a in range(3)]):
        for depth in (16, smallest_depth(dims, at)):
            for flags in FLAGS:
                check(gpu, at, list(dims), depth, flags, "scene")


def test_scene_window_hosts_the_room(scene):
    """a window on the room: every kind of node, several levels above the bricks; the tree is no trivial one"""
    gpu, c = scene
    lo, dims = [c[0] - 90, c[1] - 85, c[2] - 21], [200, 180, 40]
    for flags in (0, ref.INFL | ref.OCC_ONLY):
        got = check(gpu, lo, dims, 16, flags, "room")
        sm = got["summary"]
        assert sm[0] > 500 and sm[2] > 500 and (flags or sm[3] > 500) and sm[6] == ref.INNER
        assert (sm[8 + 1:8 + 3] > 0).all() or flags  # (free space prunes into cubes of more than one size)
    print("room summary", got["summary"])


# ---- maps built cell by cell --------------------------------------------------------------------------------------------------
def crafted(MLMap, n, d, boxes, rng):
    cfg = S1.with_(subbox_n=n, subbox_d_xyz=d)
    lo = np.min([b[1] for b in boxes], axis=0) - 3
    hi = np.max([np.add(b[0], b[1]) for b in boxes], axis=0) + 3
    r = [np.arange(lo[a] // n, (hi[a] - 1) // n + 1) for a in range(3)]
    keys = np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3)
    keys = keys[rng.random(len(keys)) < 0.85]  # (some blocks absent)
    cells = n ** 3
    occ = rng.choice(np.array([ord("o"), ord("f"), ord("u")], dtype=np.uint8), size=(len(keys), cells), p=[0.15, 0.7, 0.15])
    kind = rng.random(len(keys))
    occ[kind < 0.25] = ord("f")  # (whole blocks of one class, so that cubes above a voxel exist)
    occ[kind > 0.9] = ord("o")
    infl = np.where(rng.random(occ.shape) < 0.1, ord("o"), ord("u")).astype(np.uint8)
    gpu = MLMap(cfg, max_blocks=16384)
    assert len(keys) < 16384
    gpu.import_blocks(keys.astype(np.int32), np.zeros(occ.shape, np.float32), occ, infl, np.zeros(len(keys), np.uint8))
    return gpu


@pytest.mark.parametrize("n,d", [(2, 0.25), (3, 0.15), (16, 0.05)])
def test_crafted_maps(MLMap, n, d):
    boxes = BOXES if n == 16 else BOXES[:4]
    gpu = crafted(MLMap, n, d, boxes, np.random.default_rng(n))
    turn = 0
    for dims, lo in boxes:
        for depth in (16, smallest_depth(dims, lo)):
            for flags in (FLAGS if depth == 16 else [FLAGS[turn % 4]]):
                got = check(gpu, list(lo), list(dims), depth, flags, f"crafted n={n}")
                turn += 1
        assert got["summary"][1] > 0 or dims == (1, 1, 1)
    gpu.close()


def test_cleared_region_is_one_level_5_leaf(MLMap):
    """the aligned 32^3 region [32, 64)^3 cleared by mlm_set_free_in_bound inside noise prunes to one FREE leaf of level 5"""
    rng = np.random.default_rng(32)
    n, d = S1.subbox_n, S1.subbox_d_xyz
    lo, dims = [28, 30, 31], [40, 37, 35]
    r = [np.arange((lo[a] - 2) // n, (lo[a] + dims[a] + 1) // n + 1) for a in range(3)]
    keys = np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3)
    occ = rng.choice(np.array([ord("o"), ord("f"), ord("u")], dtype=np.uint8), size=(len(keys), n ** 3), p=[0.3, 0.4, 0.3])
    gpu = MLMap(S1, max_blocks=4096)
    gpu.import_blocks(keys.astype(np.int32), np.zeros(occ.shape, np.float32), occ, np.full(occ.shape, ord("u"), np.uint8), np.zeros(len(keys), np.uint8))
    before = check(gpu, lo, dims, 16, 0, "noise")
    assert before["summary"][8 + 3:].sum() == 0  # (noise: no cube of 8^3 or more)
    gpu.setFree_map_in_bound(np.full(3, 32.5 * d), np.full(3, 63.75 * d))  # (the voxel centres 32.5 d .. 63.5 d per axis)
    got = check(gpu, lo, dims, 16, 0, "cleared")
    assert got["summary"][8 + 5] == 1 and got["summary"][8 + 6:].sum() == 0
    at = int(np.nonzero(got["leaf4"][:, 3] == 5)[0][0])
    assert got["leaf4"][at].tolist() == [32, 32, 32, 5] and got["leaf_class"][at] == 1
    # the same cube with FREE dropped: nothing of it is left
    assert check(gpu, lo, dims, 16, ref.OCC_ONLY, "cleared, occ only")["summary"][8 + 3:].sum() == 0
    # ... and as the whole box at the smallest depth that holds it: the root's child
    got = check(gpu, [32, 32, 32], [32, 32, 32], 7, 0, "the cube alone")
    assert got["summary"].tolist()[:7] == [2, 1, 0, 1, 0, 32 ** 3, ref.INNER] and got["inner4"][:, 3].tolist() == [7, 6]
    gpu.close()


# ---- destinations, subsets, caps ----------------------------------------------------------------------------------------------
def test_destinations_subsets_and_caps(scene):
    import torch

    gpu, c = scene
    lo, dims, depth, flags = [c[0] - 20, c[1] - 19, c[2] - 9], [41, 39, 19], 16, ref.INFL
    exp = expected(gpu, lo, dims, depth, flags)
    N, M = int(exp["summary"][0]), int(exp["summary"][1])
    assert N > 50 and M > 200
    shapes = {k: (cols, dt) for k, cols, dt, _ in KEYS}
    inner = ("words", "inner4", "skip")

    def host(rows, k):
        cols, dt = shapes[k]
        a = np.empty((rows, cols) if cols > 1 else (rows,), dtype=dt)
        a.view(np.uint8).reshape(-1)[:] = SENT
        return a

    def run(names, cap_n, cap_m, device):
        arrays, keep = {}, {}
        for k in names:
            rows = cap_n if k in inner else cap_m
            if device:
                cols, dt = shapes[k]
                t = torch.full((rows * cols * np.dtype(dt).itemsize,), SENT, dtype=torch.uint8, device="cuda")
                keep[k], arrays[k] = t, t.data_ptr()
            else:
                keep[k] = arrays[k] = host(rows, k)
        if device:
            torch.cuda.synchronize()
        rc, sm = raw(gpu, lo, dims, depth, flags, arrays, cap_n if any(k in inner for k in names) else 0, cap_m if any(k not in inner for k in names) else 0)
        assert rc == 0, gpu._L.mlm_last_error(gpu._h)
        assert np.array_equal(sm, exp["summary"])  # (the summary tells the truth whatever the caps)
        for k in names:
            total, cap = (N, cap_n) if k in inner else (M, cap_m)
            rows = min(total, cap)
            b = keep[k].cpu().numpy().tobytes() if device else keep[k].tobytes()
            size = len(b) // max(cap, 1)
            assert b[:rows * size] == exp[k][:rows].tobytes(), (names, cap_n, cap_m, device, k)
            assert (np.frombuffer(b[rows * size:], dtype=np.uint8) == SENT).all(), (names, cap_n, cap_m, device, k, "rows beyond the cap were written")

    for device in (False, True):
        run([k for k, _, _, _ in KEYS], N, M, device)  # all together
        for k, _, _, _ in KEYS:  # each alone
            run([k], N + 3, M + 3, device)
        for cap_n, cap_m in ((1, 1), (N - 1, M - 1), (N + 5, 1), (1, M + 5)):  # caps that clip
            run([k for k, _, _, _ in KEYS], cap_n, cap_m, device)
        run(["words", "leaf_class"], N - 1, M - 1, device)
    # mixed: inner rows to the device, leaves to the host
    w = torch.full((N,), 0x7777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    leaf4 = host(M, "leaf4")
    rc, sm = raw(gpu, lo, dims, depth, flags, {"words": w.data_ptr(), "leaf4": leaf4}, N, M, summary=False)
    assert rc == 0 and w.cpu().numpy().view(np.uint16).tobytes() == exp["words"].tobytes() and leaf4.tobytes() == exp["leaf4"].tobytes()
    # the binding's device call
    sk = torch.zeros(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sm = gpu.export_octree_dev(lo, dims, depth, infl=True, skip=sk.data_ptr(), cap_inner=N)
    assert np.array_equal(sm, exp["summary"]) and np.array_equal(sk.cpu().numpy(), exp["skip"])
    assert gpu.export_octree_dev(lo, dims, depth, infl=True, skip=sk.data_ptr(), cap_inner=N, summary=False) is None


def test_host_rows_beyond_one_staged_range(MLMap):
    """a 128^3 checkerboard: every voxel a leaf, 2^21 of them — host destinations are staged in ranges of 2^20 rows, so the leaves
    take two.  The expected rows are closed forms: the voxels in Morton order, the class their parity; one word for every level-1
    cell, 0xFFFF above, and a chain of single-child nodes from level 8 to the root."""
    n, side = S1.subbox_n, 128
    nb = -(-side // n)
    keys = np.stack(np.meshgrid(*[np.arange(nb)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cz, cy, cx = np.unravel_index(np.arange(n ** 3), (n, n, n))
    parity = (keys.sum(axis=1)[:, None] * n + (cx + cy + cz)[None, :]) & 1
    occ = np.where(parity == 0, ord("o"), ord("f")).astype(np.uint8)
    gpu = MLMap(S1, max_blocks=4096)
    gpu.import_blocks(keys.astype(np.int32), np.zeros(occ.shape, np.float32), occ, np.full(occ.shape, ord("u"), np.uint8), np.zeros(len(keys), np.uint8))
    got = gpu.export_octree([0, 0, 0], [side] * 3, 16)
    M = side ** 3
    levels = [8 ** k for k in range(7)]  # cells of levels 7..1 of the cube
    assert M == 2 << 20 and got["summary"].tolist()[:8] == [sum(levels) + 9, M, M // 2, M // 2, M // 2, M // 2, ref.INNER, 0]
    assert got["summary"][8] == M and got["summary"][9:].sum() == 0
    # the leaves: Morton order of (x, y, z), x lowest
    z, y, x = np.unravel_index(np.arange(M), (side,) * 3)
    code = np.zeros(M, dtype=np.int64)
    for b in range(7):
        code |= ((x >> b) & 1) << (3 * b) | ((y >> b) & 1) << (3 * b + 1) | ((z >> b) & 1) << (3 * b + 2)
    order = np.argsort(code)
    exp4 = np.stack([x[order], y[order], z[order], np.zeros(M, dtype=np.int64)], axis=1).astype(np.int32)
    assert got["leaf4"].tobytes() == exp4.tobytes()
    assert got["leaf_class"].tobytes() == ((x + y + z)[order] & 1).astype(np.int8).tobytes()
    # the words
    w1 = sum((ref.OCC if bin(i).count("1") % 2 == 0 else ref.FREE) << (2 * i) for i in range(8))
    lv = got["inner4"][:, 3]
    assert (got["words"][lv == 1] == w1).all() and (lv == 1).sum() == levels[6]
    assert (got["words"][(lv >= 2) & (lv <= 7)] == 0xFFFF).all() and ((lv >= 2) & (lv <= 7)).sum() == sum(levels[:6])
    assert lv[:9].tolist() == list(range(16, 7, -1)) and got["words"][:9].tolist() == [3 << 14] + [3] * 8  # (key 2^15: the root's child 7, then child 0)
    assert np.array_equal(got["skip"][:10], np.full(10, len(lv))) and got["skip"][-1] == len(lv)
    gpu.close()


def test_empty_map_and_default_box(MLMap):
    gpu = MLMap(S1, max_blocks=1024)
    got = gpu.export_octree([-20, -3, 5], [50, 40, 30])
    assert not got["summary"].any() and all(len(got[k]) == 0 for k, _, _, _ in KEYS)  # N = M = 0, the root's label NONE
    got = gpu.export_octree()  # (no block: a box of one voxel)
    assert not got["summary"].any()
    # one block of FREE voxels: the default box is the block
    n = S1.subbox_n
    gpu.import_blocks(np.array([[2, -1, 0]], dtype=np.int32), np.zeros((1, n ** 3), np.float32), np.full((1, n ** 3), ord("f"), np.uint8),
                      np.full((1, n ** 3), ord("u"), np.uint8), np.zeros(1, np.uint8))
    got = gpu.export_octree()
    assert got["lo"].tolist() == [2 * n, -n, 0] and got["dims"].tolist() == [n, n, n] and got["summary"][5] == n ** 3 and got["summary"][4] == 0
    same(got, expected(gpu, got["lo"].tolist(), got["dims"].tolist(), 16, 0), "default box")
    gpu.close()


def test_second_call_after_more_frames_reuses_the_scratch(MLMap):
    gpu = MLMap(S1, max_blocks=16384)
    stream = list(syn.stream(S1, "room_jitter", "smooth", 6))
    for img, (q, t) in stream[:3]:
        gpu.update_map(img, q, t)
    n = S1.subbox_n
    small, large = ([-30, -25, -10], [60, 50, 20]), ([-70, -66, -15], [150, 131, 40])
    base = gpu.frame_stats()["device_bytes"]
    first = check(gpu, *large, 16, 0, "first")
    grown = gpu.frame_stats()["device_bytes"]
    assert grown > base  # (the scratch and the staging are the handle's, and counted)
    check(gpu, *small, 16, ref.INFL, "smaller box, same scratch")
    assert gpu.frame_stats()["device_bytes"] == grown
    for img, (q, t) in stream[3:]:
        gpu.update_map(img, q, t)
    second = check(gpu, *large, 16, 0, "after more frames")
    assert gpu.frame_stats()["device_bytes"] == grown or second["summary"][0] > first["summary"][0]
    assert not np.array_equal(first["summary"], second["summary"])  # (the map has changed, and the tree with it)
    assert n == 10
    gpu.close()


def test_frontier_mode_released_blocks(MLMap):
    """a frontier-mode handle with inflation: released blocks answer from element 0 (the window's rule)"""
    cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
    gpu = MLMap(cfg, max_blocks=16384, max_batch=2)
    for k, (img, (q, t)) in enumerate(syn.stream(cfg, "room_jitter", "smooth", 8)):
        gpu.update_map(img, q, t)
        if k in (3, 6):
            gpu.inflate_map(t)
    b = gpu.export_blocks()
    assert b["collapsed"].sum() > 20
    n = cfg.subbox_n
    lo = [int(v) for v in b["keys"].min(0) * n - 7]
    dims = [min(int(v), 80) for v in (b["keys"].max(0) + 2) * n - 4 - np.array(lo)]
    for flags in (0, ref.INFL):
        assert check(gpu, lo, dims, 16, flags, "frontier mode")["summary"][0] > 100
    gpu.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(scene):
    from mlmapping_amd.mlmap import MlmError

    gpu, c = scene
    lo, dims = [c[0] - 5, c[1] - 5, c[2] - 5], [11, 12, 13]
    good = gpu.export_octree(lo, dims)
    INVALID = -1
    w, l4 = np.zeros(4, dtype=np.uint16), np.zeros((4, 4), dtype=np.int32)
    cases = [
        (lo, [0, 5, 5], 16, 0, {}, 0, 0, True),                   # the window's own errors
        ([2 ** 31 - 4, 0, 0], [5, 1, 1], 31, 0, {}, 0, 0, True),
        ([-1000, -1000, -1000], [2000, 2000, 2000], 16, 0, {}, 0, 0, True),  # more than 2^31 - 1 voxels
        (lo, dims, 0, 0, {}, 0, 0, True), (lo, dims, 32, 0, {}, 0, 0, True),  # depth
        ([-64, 0, 0], [129, 1, 1], 7, 0, {}, 0, 0, True), ([32767, 0, 0], [2, 1, 1], 16, 0, {}, 0, 0, True),  # outside the key cube
        (lo, dims, 16, 4, {}, 0, 0, True), (lo, dims, 16, -1, {}, 0, 0, True),  # an unknown flag bit
        (lo, dims, 16, 0, {"words": w}, -1, 0, True),             # a negative cap
        (lo, dims, 16, 0, {"words": w}, 0, 0, True), (lo, dims, 16, 0, {}, 4, 0, True),  # a cap at odds with its arrays
        (lo, dims, 16, 0, {"leaf4": l4}, 0, 0, True), (lo, dims, 16, 0, {}, 0, 4, True),
        (lo, dims, 16, 0, {}, 0, 0, False),                       # no output
    ]
    for lo_, dims_, depth, flags, arrays, cap_n, cap_m, summary in cases:
        rc, _ = raw(gpu, lo_, dims_, depth, flags, arrays, cap_n, cap_m, summary)
        assert rc == INVALID, (lo_, dims_, depth, flags, cap_n, cap_m, summary)
        assert b"mlm_export_octree" in gpu._L.mlm_last_error(gpu._h)
        same(gpu.export_octree(lo, dims), good, "after a refused call")
    with pytest.raises(MlmError):
        gpu.export_octree(lo, dims, depth=40)
    # the key cube's two ends at depth 7 are fine
    rc, sm = raw(gpu, [-64, 0, 0], [128, 1, 1], 7, 0, {}, 0, 0)
    assert rc == 0
