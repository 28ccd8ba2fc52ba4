"""mlm_score_poses: exact scan-to-map scores of candidate poses (include/mlmap_hip.h), every word of every row held to the contract
written in numpy (tests/score_ref.py) over classes that do not come from the code under test: maps built voxel by voxel, random
block dumps, and the CPU oracle's block dump.  Every case runs three ways — host memory (small batches: the host code, with classes
through the host mirror), device tensors for every pointer (the kernel k_score), and host memory again after
set_host_mirror_limit(0) (the kernel, staged) — and all three must give the reference's bytes.  The table is filled with garbage
before every call and every call is made twice: the path that adds with atomics must not accumulate across calls."""
import ctypes
import math

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import esdf_ref as er
from tests import raywalk_ref as rw
from tests import score_ref as sc
from tests.test_gpu_nearest import centre, dump, load, random_dump, to_numpy

pytestmark = pytest.mark.gpu

D, N = S1.subbox_d_xyz, S1.subbox_n
SX = S1.with_(use_exploration_frontiers=True)  # released blocks answer from element 0 only in frontier mode
TILE = 128            # points per LDS tile of k_score (MLM_SCORE_TILE, mlm_kernels_score.h); score_chunk is a multiple of it
MANY = 3 * TILE + 5
HOST_PAIRS = 1 << 16  # the host code answers n_poses * n_pts <= 2^16 pairs of at most 64 poses (include/mlmap_hip.h)
HOST_POSES = 64
GARBAGE = -0x0123456789ABCDEF
CUBE3 = [(gx, gy, gz) for gx in (-1, 0, 1) for gy in (-1, 0, 1) for gz in (-1, 0, 1)]  # voxels -10 .. 19 on every axis


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def box_voxels(lo, dims):
    iz, iy, ix = np.unravel_index(np.arange(int(np.prod(dims))), (dims[2], dims[1], dims[0]))
    return np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)


def esdf_field(classes, lo, dims, C, signed=False):
    """mlm_export_esdf's sqdist over the box (OCC), from the classes of the box grown by C"""
    glo, gd = er.grown([int(v) for v in lo], [int(v) for v in dims], C)
    mask = ((classes(box_voxels(glo, gd)) & sc.OCC) != 0).reshape(gd[2], gd[1], gd[0])
    return np.ascontiguousarray(er.expected(mask, C, signed, 1.0)["sqdist"], dtype=np.int32)


def wild_field(rng, dims):
    f = rng.integers(-(1 << 31), 1 << 31, size=(int(dims[2]), int(dims[1]), int(dims[0])), dtype=np.int64).astype(np.int32)
    small = rng.random(f.shape) < 0.5
    f[small] = rng.integers(-3, 70, size=int(small.sum()))
    f.reshape(-1)[:4] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0, -1]
    return f


def call(gpu, pts, T, classes, box, field, cap, where):
    """one call through score_poses_dev into a table filled with garbage; where: "host", "dev" (every pointer a device tensor) or
    "field_host" (sqdist in host memory, everything else on the device)"""
    import torch

    pts, T = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 12)
    lo, dims = box if box is not None else (None, None)
    f = None if field is None else np.ascontiguousarray(field, dtype=np.int32)
    if where == "host":
        table = np.full((len(T), sc.ROW), GARBAGE, dtype=np.int64)
        gpu.score_poses_dev(pts.ctypes.data if len(pts) else None, len(pts), T.ctypes.data, len(T), table.ctypes.data, classes, lo, dims,
                            None if f is None else f.ctypes.data, cap)
        return table
    p, t = torch.from_numpy(pts).cuda(), torch.from_numpy(T).cuda()
    table = torch.full((len(T), sc.ROW), GARBAGE, dtype=torch.int64, device="cuda")
    fd = None if f is None or where == "field_host" else torch.from_numpy(f).cuda()
    fp = None if f is None else (f.ctypes.data if fd is None else fd.data_ptr())
    gpu.score_poses_dev(p.data_ptr() if len(pts) else None, len(pts), t.data_ptr(), len(T), table.data_ptr(), classes, lo, dims, fp, cap)
    return table.cpu().numpy()


def warm(gpu):
    """one answer from the host mirror: it is up to date from here on, and batches of up to 64 poses qualify"""
    t = call(gpu, centre([0, 0, 0]), sc.IDENTITY, True, None, None, 64, "host")
    assert t[0, 0] == 1


def three_ways(make, cases, d=D):
    """cases: [(pts, T, classes callable or None, box or None, field or None, sq_cap, expected table)] on the map make() builds"""
    gpu = make()
    warm(gpu)
    for i, (p, T, cl, box, f, cap, exp) in enumerate(cases):
        T = np.asarray(T, dtype=np.float64).reshape(-1, 12)
        on_host = cl is not None and len(T) <= HOST_POSES and len(T) * len(p) <= HOST_PAIRS
        for rep in range(2):
            before = gpu.frame_stats()["n_host_queries"]
            sc.assert_equal(call(gpu, p, T, cl is not None, box, f, cap, "host"), exp, f"case {i} host memory, call {rep}")
            if cl is not None:
                assert gpu.frame_stats()["n_host_queries"] == before + (len(T) if on_host else 0), (i, len(T), len(p))
            sc.assert_equal(call(gpu, p, T, cl is not None, box, f, cap, "dev"), exp, f"case {i} device tensors, call {rep}")
        if f is not None:
            sc.assert_equal(call(gpu, p, T, cl is not None, box, f, cap, "field_host"), exp, f"case {i} sqdist in host memory")
    gpu.close()
    gpu = make()
    gpu.set_host_mirror_limit(0)
    for i, (p, T, cl, box, f, cap, exp) in enumerate(cases):
        for rep in range(2):
            sc.assert_equal(call(gpu, p, T, cl is not None, box, f, cap, "host"), exp, f"case {i} staged kernel, call {rep}")
    assert gpu.frame_stats()["n_host_queries"] == 0
    gpu.close()


def modes(p, T, classes, box, f, cap, d=D):
    """the three modes of one input: classes only, field only, both — each with its reference"""
    return [(p, T, classes, None, None, cap, sc.score(p, T, d, classes)),
            (p, T, None, box, f, cap, sc.score(p, T, d, None, box, f, cap)),
            (p, T, classes, box, f, cap, sc.score(p, T, d, classes, box, f, cap))]


def scan(rng, n, d, n_pts, n_poses):
    ext = (3 * n + 2) * d
    pts = rng.uniform(-0.6 * ext, 0.6 * ext, size=(n_pts, 3))
    T = np.concatenate([sc.random_rotations(rng, n_poses), rng.uniform(-0.5 * ext, 0.5 * ext, size=(n_poses, 3))], axis=1)
    return pts, T


# ---- answers written by hand, edges of the box, absent and released blocks --------------------------------------------------------
def test_by_hand_and_box_edges(mods):
    """one obstacle; per axis the voxels lo - 1, lo, lo + dims - 1 and lo + dims, among negative coordinates"""
    MLMap, _ = mods
    b = dump([(3, 0, 0)], CUBE3, inflated=[(3, 0, 0)])
    classes = rw.block_classes(b, N)
    # a quarter turn about z plus half a voxel: s = (0, -3, 0) d -> w = (3.5, 0.5, 0.5) d, voxel (3, 0, 0): the obstacle, field -4;
    # s = (1, 0, 2) d -> w = (0.5, 1.5, 2.5) d, voxel (0, 1, 2): free, field 7
    quarter = np.array([0.0, -1, 0, 1, 0, 0, 0, 0, 1, 0.5 * D, 0.5 * D, 0.5 * D])
    f = np.full((3, 2, 4), 50, dtype=np.int32)  # box lo (0, 0, 0), dims (4, 2, 3)
    f[0, 0, 3], f[2, 1, 0] = -4, 7
    p = np.array([[0, -3 * D, 0], [D, 0, 2 * D]])
    hand = sc.score(p, quarter, D, classes, ([0, 0, 0], [4, 2, 3]), f, 9)
    assert hand.tolist() == [[2, 1, 1, 0, 1, 2, 7, 1]]
    lo, dims = np.array([-7, -3, 2]), np.array([5, 9, 4])
    rng = np.random.default_rng(1)
    g = wild_field(rng, dims)
    edge = []
    for a in range(3):
        for k in (lo[a] - 1, lo[a], lo[a] + dims[a] - 1, lo[a] + dims[a]):
            v = lo + dims // 2
            v[a] = k
            edge.append(v)
    pe = centre(edge)
    exp = sc.score(pe, sc.IDENTITY, D, classes, (lo, dims), g, 1 << 20)
    assert exp[0, 0] == 12 and exp[0, 5] == 6
    one_by_one = [(pe[i:i + 1], sc.IDENTITY, classes, (lo, dims), g, 1 << 20, sc.score(pe[i:i + 1], sc.IDENTITY, D, classes, (lo, dims), g, 1 << 20))
                  for i in range(12)]
    assert [int(c[6][0, 5]) for c in one_by_one] == [0, 1, 1, 0] * 3
    three_ways(lambda: load(MLMap, b), [(p, quarter, classes, ([0, 0, 0], [4, 2, 3]), f, 9, hand), (pe, sc.IDENTITY, classes, (lo, dims), g, 1 << 20, exp)]
               + one_by_one + modes(pe, sc.IDENTITY, classes, (lo, dims), g, 1))


def test_absent_and_released_blocks(mods):
    """frontier mode: points inside released blocks whose element 0 is 'o', 'f' and 'u', inside an absent block, beyond the key range"""
    MLMap, _ = mods
    rel = {(2, 0, 0): "o", (0, 2, 0): "f", (0, 0, 2): "u"}
    b = dump([(5, 5, 5)], [(0, 0, 0), (1, 0, 0)], inflated=[(7, 7, 7)], unknown=[(1, 1, 1)], released=rel)
    classes = rw.block_classes(b, N)
    vox = [(25, 5, 5), (29, 0, 9), (5, 25, 5), (5, 5, 25), (5, 5, 5), (7, 7, 7), (1, 1, 1), (2, 2, 2), (-5, -5, -5), (15, 15, 15)]
    p = np.concatenate([centre(vox), [[3.0e6 * D * N, 0.5 * D, 0.5 * D]]])  # (the last one a million blocks out: UNKNOWN)
    each = [sc.score(p[i:i + 1], sc.IDENTITY, D, classes)[0, 1:5].tolist() for i in range(len(p))]
    assert each == [[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 1, 0],
                    [0, 0, 1, 0], [0, 0, 1, 0]]
    lo, dims = np.array([-6, -6, -6]), np.array([40, 40, 40])
    f = esdf_field(classes, lo, dims, 8, signed=True)
    T = np.stack([sc.IDENTITY, np.concatenate([sc.IDENTITY[:9], [D, 0, 0]]), np.concatenate([sc.IDENTITY[:9], [0, -3 * D, 2 * D]])])
    three_ways(lambda: load(MLMap, b, SX), modes(p, T, classes, (lo, dims), f, 64))


# ---- shapes: pose groups, LDS tiles, chunks ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shaped():
    """one map and one scan of 257 poses x 3 tile + 5 points (with invalid pairs); the reference per point count, all three modes"""
    rng = np.random.default_rng(8)
    b = random_dump(rng, N)
    b["collapsed"][:] = 0
    classes = rw.block_classes(b, N)
    pts, T = scan(rng, N, D, MANY, 257)
    pts[5], pts[TILE], pts[MANY - 1, 2] = [np.nan, 0, 0], [0, np.inf, 0], 1e300
    T[7, 3], T[200, 11] = np.nan, -np.inf
    lo, dims = np.full(3, -2 * N), np.array([4 * N + 3, 4 * N + 1, 3 * N + 2])
    f = esdf_field(classes, lo, dims, 8)
    ref = {m: modes(pts[:m], T, classes, (lo, dims), f, 64) for m in (0, 1, TILE - 1, TILE, TILE + 1, MANY)}
    assert ref[MANY][2][6][:, 0].max() == MANY - 3 and not ref[MANY][2][6][7].any() and not ref[MANY][2][6][200].any()
    return b, ref


def subset(case, n_poses):
    p, T, cl, box, f, cap, exp = case
    return (p, T[:n_poses], cl, box, f, cap, exp[:n_poses])


@pytest.mark.parametrize("n_poses", [1, 63, 64, 65, 257])
def test_pose_groups_and_point_tiles(mods, shaped, n_poses):
    """every point count around the LDS tile with the automatic chunk (one tile per chunk here: 3 tile + 5 points add with atomics)"""
    MLMap, _ = mods
    b, ref = shaped
    three_ways(lambda: load(MLMap, b), [subset(c, n_poses) for m in ref for c in ref[m]])


@pytest.mark.parametrize("chunk,chunks", [(4 * TILE, 1), (2 * TILE, 2), (TILE, 4)])
def test_store_path_and_atomic_path(mods, shaped, knobs, chunk, chunks):
    """score_chunk forces one chunk (plain stores), two and four (atomics) for 3 tile + 5 points"""
    MLMap, _ = mods
    b, ref = shaped
    assert (MANY + chunk - 1) // chunk == chunks
    knobs.set("score_chunk", chunk)
    three_ways(lambda: load(MLMap, b), [subset(c, k) for k in (1, 65, 257) for c in ref[MANY]] + [subset(c, 257) for c in ref[TILE + 1]])


def test_score_chunk_knob_is_checked():
    from mlmapping_amd import mlmap

    L = mlmap.load_library()
    for bad in (1, TILE - 1, TILE + 1, -TILE, (1 << 22) + TILE):
        assert L.mlm_debug_set(b"score_chunk", ctypes.c_longlong(bad)) == -1
    for ok in (0, TILE, 1 << 22):
        assert L.mlm_debug_set(b"score_chunk", ctypes.c_longlong(ok)) == 0
    mlmap.debug_reset()


# ---- random maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["n10", "n5 with released blocks"])
def test_random_maps(mods, which):
    """257 poses x 3 tile + 5 points over a random dump; signed and arbitrary int32 fields, sq_cap 1, 64 and 2^20"""
    MLMap, _ = mods
    cfg = S1 if which == 0 else SX.with_(subbox_n=5)
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    rng = np.random.default_rng(41 + which)
    b = random_dump(rng, n, nblk=150 if which else 40)
    r = rng.random(b["occ"].shape)
    b["occ"] = np.where(r < 0.02, ord("o"), np.where(r < 0.07, ord("u"), ord("f"))).astype(np.uint8)  # (test_score_plan's densities)
    b["infl"] = np.where(rng.random(b["occ"].shape) < 0.03, ord("o"), ord("u")).astype(np.uint8)
    if which == 0:
        b["collapsed"][:] = 0
    else:
        b["occ"][b["collapsed"].astype(bool), 0] = rng.choice([ord("f"), ord("u"), ord("o")], size=int(b["collapsed"].sum()))
    classes = rw.block_classes(b, n)
    pts, T = scan(rng, n, d, MANY, 257)
    lo, dims = np.full(3, -2 * n), np.array([4 * n + 3, 4 * n + 1, 3 * n + 2])
    unsigned, signed, wild = esdf_field(classes, lo, dims, 8), esdf_field(classes, lo, dims, 8, signed=True), wild_field(rng, dims)
    cases = modes(pts, T, classes, (lo, dims), unsigned, 64)
    tot = sc.non_vacuous(cases[2][6], f"which={which}")
    print(f"n={n}: [1] {tot[1]} [2] {tot[2]} [3] {tot[3]} [4] {tot[4]} [5] / [0] {tot[5]} / {tot[0]}")
    for f, cap in ((signed, 1), (wild, 1 << 20), (wild, 1)):
        cases.append((pts, T, classes, (lo, dims), f, cap, sc.score(pts, T, d, classes, (lo, dims), f, cap)))
    three_ways(lambda: load(MLMap, b, cfg), cases, d)


# ---- the oracle's scene -------------------------------------------------------------------------------------------------------------
SCENE_Q, SCENE_T = syn.quat_from_rpy(0.02, -0.03, math.radians(30.0)), np.array([0.37, -0.21, 1.43])
HALF, YAWS = (3, 3, 1), (-2, -1, 0, 1, 2)


@pytest.fixture(scope="module")
def scene(mods):
    """S1, four frames of the synthetic room at one pose, on the library and on the oracle; the frame's points at step 8, the grid of
    735 poses around the integration pose, the box around the points, and the reference's field and table on the oracle's dump"""
    from mlmapping_amd.mlmap import backproject, compose_T_ws, pose_grid

    MLMap, OracleMap = mods
    img = syn.room_depth(S1)
    gpu, cpu = MLMap(S1, max_blocks=8192), OracleMap(S1)
    for _ in range(4):
        gpu.update_map(img, SCENE_Q, SCENE_T)
        cpu.update_depth(img, SCENE_Q, SCENE_T)
    classes = rw.block_classes(cpu.export_blocks(), N)
    pts = backproject(img, (S1.cam_fx, S1.cam_fy, S1.cam_cx, S1.cam_cy), 8)
    T0 = compose_T_ws(SCENE_Q[None], SCENE_T[None], S1.T_B_S)[0]
    grid = pose_grid(T0, D, HALF, YAWS)
    assert pts.shape == (4800, 3) and grid.shape == (735, 12)
    v = sc.voxels(sc.world(pts, T0), D)[1][0]
    lo, dims = v.min(0) - 6, v.max(0) - v.min(0) + 13
    field = esdf_field(classes, lo, dims, 8)
    table = sc.score(pts, grid, D, classes, (lo, dims), field, 64)
    yield gpu, pts, grid, lo, dims, field, table
    gpu.close()


def grid_offsets():
    """(yaw in degrees, ix, iy, iz) of every row of pose_grid(.., HALF, YAWS)"""
    nx, ny, nz = (2 * h + 1 for h in HALF)
    i = np.arange(len(YAWS) * nx * ny * nz)
    return np.array(YAWS)[i // (nx * ny * nz)], i % nx - HALF[0], i // nx % ny - HALF[1], i // (nx * ny) % nz - HALF[2]


def test_scene_recovers_the_integration_pose(scene):
    """Asserted on the reference's table (the oracle's map, tests/score_ref.py), not on the code under test: the row with the smallest
    [6] lies near the pose the frames were integrated at, and its [6] is smaller than at every pose on the border of the grid.
    Measured on the CPU with the oracle: the argmin sits at (+1 deg, +1, -2, 0) voxels from the integration pose, cost 483 against
    612 at that pose; the smallest cost on the border is 506.  The basin is flat because the map is blurred by the sensor model's
    radial spread and by the 1-degree awareness cells, not by the call, so the tolerance is the measured offset plus one voxel per
    axis and one yaw step: |yaw| <= 2 deg, |x| <= 2, |y| <= 3, |z| <= 1 voxels."""
    table = scene[6]
    yaw, ix, iy, iz = grid_offsets()
    best = sc.best_row(table)
    truth = int(np.flatnonzero((yaw == 0) & (ix == 0) & (iy == 0) & (iz == 0))[0])
    print(f"argmin {best}: yaw {yaw[best]} offset ({ix[best]}, {iy[best]}, {iz[best]}) cost {table[best, 6]}; at the integration pose {table[truth, 6]}")
    assert abs(yaw[best]) <= 2 and abs(ix[best]) <= 2 and abs(iy[best]) <= 3 and abs(iz[best]) <= 1
    border = (np.abs(ix) == HALF[0]) | (np.abs(iy) == HALF[1]) | (np.abs(iz) == HALF[2]) | (yaw == YAWS[0]) | (yaw == YAWS[-1])
    assert not border[best] and (table[border, 6] > table[best, 6]).all(), (table[best, 6], table[border, 6].min())
    assert table[best, 1] == table[:, 1].max() and table[best, 7] == table[:, 7].max()  # ([1] and the zero-cost count pick the same row)


def test_scene_match_pose(scene):
    """the library's field equals esdf_ref on the oracle's dump; match_pose equals the reference, table and index, and equals
    score_poses with the field passed by hand"""
    import torch

    gpu, pts, grid, lo, dims, field, table = scene
    got_field = gpu.export_esdf(lo, dims, 8)["sqdist"]
    assert got_field.dtype == np.int32 and np.array_equal(got_field, field)
    for cl in (True, False):
        exp = table.copy()
        if not cl:
            exp[:, 1:5] = 0
        m = gpu.match_pose(pts, grid, lo, dims, 8, classes=cl)
        sc.assert_equal(m["table"], exp, f"match_pose classes={cl}")
        assert m["best"] == sc.best_row(exp) and np.array_equal(m["cost"], exp[:, 6])
        by_hand = gpu.score_poses(pts, grid, cl, (lo, dims), got_field, 64)
        sc.assert_equal(by_hand["table"], exp, f"score_poses, the field by hand, classes={cl}")
        dev = gpu.match_pose(torch.from_numpy(pts).cuda(), torch.from_numpy(grid).cuda(), lo, dims, 8, classes=cl)
        sc.assert_equal(dev["table"].cpu().numpy(), exp, f"match_pose on tensors classes={cl}")
        assert dev["best"] == m["best"]


def test_async_mode(mods):
    """after update_map_batch in async mode, without sync(): with classes the call sees every submitted frame; a field-only call
    succeeds and equals the reference too"""
    MLMap, OracleMap = mods
    nf = 4
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(S1, max_blocks=8192, max_batch=4), OracleMap(S1)
    for k in range(nf):
        cpu.update_depth(frames[k], q[k], t[k])
    b = cpu.export_blocks()
    classes = rw.block_classes(b, N)
    rng = np.random.default_rng(2)
    klo, khi = b["keys"].min(0) * N * D, (b["keys"].max(0) + 1) * N * D
    pts = rng.uniform(-1.5, 1.5, size=(300, 3))
    T = np.concatenate([sc.random_rotations(rng, 70), rng.uniform(klo, khi, size=(70, 3))], axis=1)
    lo, dims = np.array([0, 0, 0]), np.array([30, 20, 10])
    f = wild_field(rng, dims)
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    sc.assert_equal(call(gpu, pts, T, False, (lo, dims), f, 64, "host"), sc.score(pts, T, D, None, (lo, dims), f, 64), "async, field only")
    exp = sc.score(pts, T, D, classes, (lo, dims), f, 64)
    assert exp[:, 1].sum() >= 20 and exp[:, 2].sum() >= 200
    sc.assert_equal(call(gpu, pts, T, True, (lo, dims), f, 64, "host"), exp, "async, classes")
    gpu.close()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_arguments(mods, knobs):
    MLMap, _ = mods
    b = dump([(3, 0, 0)], CUBE3)
    for mirror in (1, 0):
        knobs.set("mirror", mirror)
        gpu = load(MLMap, b)
        L, h = gpu._L, gpu._h
        P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        pts = np.ascontiguousarray(centre([(3, 0, 0), (0, 3, 0)]))
        T = np.ascontiguousarray(np.stack([sc.IDENTITY, sc.IDENTITY]))
        lo, dims = np.array([0, 0, 0], np.int32), np.array([4, 4, 1], np.int32)
        f = np.arange(16, dtype=np.int32)
        table = np.zeros((2, 8), np.int64)
        call_ = lambda p=pts, m=2, t=T, n=2, fl=1, l=lo, d=dims, s=f, cap=64, out=table: L.mlm_score_poses(h, P(p), m, P(t), n, fl, P(l), P(d), P(s), cap, P(out))
        big = np.array([2 ** 31 - 4, 0, 0], np.int32)
        for bad in (lambda: call_(m=-1), lambda: call_(m=(1 << 22) + 1), lambda: call_(n=-1), lambda: call_(n=(1 << 22) + 1), lambda: call_(p=None),
                    lambda: call_(t=None), lambda: call_(out=None), lambda: call_(n=0, out=None), lambda: call_(fl=2), lambda: call_(fl=3),
                    lambda: call_(fl=-1), lambda: call_(fl=0, l=None, d=None, s=None), lambda: call_(l=None), lambda: call_(d=None),
                    lambda: call_(s=None), lambda: call_(l=None, d=None), lambda: call_(cap=0), lambda: call_(cap=(1 << 20) + 1), lambda: call_(cap=-5),
                    lambda: call_(d=np.array([4, 0, 1], np.int32)), lambda: call_(l=big), lambda: call_(d=np.array([2048, 2048, 2048], np.int32))):
            assert bad() == -1
            assert call_() == 0  # (the handle is usable afterwards)
        assert call_(n=0, t=None) == 0 and call_(fl=1, l=None, d=None, s=None, cap=0) == 0  # (n_poses == 0; sq_cap is not read without a field)
        table[...] = 9
        assert call_() == 0
        assert table.tolist() == [[2, 1, 1, 0, 0, 2, 15, 0]] * 2  # (voxel (3, 0, 0): f = 3; (0, 3, 0): f = 12)
        table[...] = 9
        assert call_(p=None, m=0) == 0 and not table.any()  # (n_pts == 0 writes zero rows)
        table[...] = 9
        assert call_(fl=0) == 0 and table.tolist() == [[2, 0, 0, 0, 0, 2, 15, 0]] * 2
        gpu.close()
