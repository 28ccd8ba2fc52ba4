"""mlm_query_sweeps: exact segment casts for a ball of robot radius (include/mlmap_hip.h), every output held byte for byte to the
contract written in plain Python integers (tests/sweep_ref.py: the full ball at every path voxel, no caps) over classes that do not
come from the code under test: maps built voxel by voxel, and the CPU oracle's block dump.  Every case runs three ways — small batches
in host memory (the host mirror), device tensors for every pointer (the kernels k_sweeps0 / k_sweeps), and host memory again after
set_host_mirror_limit(0) (the kernels, staged) — and all three must give the same bytes.  The shapes are the smallest at which the
kernel can go wrong: column tables that do not divide 64, obstacles on the sphere and just outside it, ties that enter the cap in one
step, block layers that enter the slot cache at the last crossing, released and absent blocks, and the geometry (subbox_n 5, radius
11 and 16) whose block box does not fit the cache and is probed per lane."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import raywalk_ref as rw
from tests import sweep_ref as sr
from tests.test_gpu_nearest import CUBE3, at, centre, dump, kw, load, random_dump, to_numpy

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN = sr.OCC, sr.INFL, sr.UNKNOWN
D, N = S1.subbox_d_xyz, S1.subbox_n
SX = S1.with_(use_exploration_frontiers=True)  # released blocks answer from element 0 only in frontier mode
S5 = SX.with_(subbox_n=5)
SWEEP_CHUNK = 1 << 18    # rays per launch when host memory is staged (include/mlmap_hip.h: "93 bytes x 2^18 rays")
MIRROR_VOXELS = 1 << 18  # the mirror's bound on the sum of (2r + 1)^3 + N L(r)


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def blocks(lo, hi):
    return [(gx, gy, gz) for gx in range(lo, hi) for gy in range(lo, hi) for gz in range(lo, hi)]


def through_mirror(gpu, p0, p1, r, flags, d):
    """the batch in host memory in pieces the mirror takes (at most 8 rays at first: the mirror needs a refresh; then 64; the sum of
    (2r + 1)^3 + N L(r) within the bound); a ray beyond the bound on its own must not be answered on the host"""
    work = [(2 * r + 1) ** 3 + (sr.path_len(a, b, d) - 1) * sr.columns(r) if sr.path_len(a, b, d) else 0 for a, b in zip(p0, p1)]
    parts, i, clean = [], 0, False
    while i < len(p0):
        m, tot = 0, 0
        while i + m < len(p0) and m < (64 if clean else 8) and tot + work[i + m] <= MIRROR_VOXELS:
            tot += work[i + m]
            m += 1
        before = gpu.frame_stats()["n_host_queries"]
        parts.append(gpu.query_sweeps(p0[i:i + max(m, 1)], p1[i:i + max(m, 1)], r, **kw(flags)))
        after = gpu.frame_stats()["n_host_queries"]
        if m:
            assert after == before + m, "the batch was not answered by the host mirror"
            clean = True
        else:
            assert after == before, "a batch beyond the mirror's bound was answered on the host"
        i += max(m, 1)
    return {k: np.concatenate([p[k] for p in parts]) for k in sr.OUTPUTS}


def three_ways(make, cases, classes, d=D):
    """cases: [(p0, p1, flags, r)] on the map make() builds: mirror and device tensors on one handle, then the kernel with staged host
    memory on a handle after set_host_mirror_limit(0); everything equal to sweep_ref.  Returns the reference's answers."""
    import torch

    cases = [(np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3), f, r)
             for a, b, f, r in cases]
    exp = [sr.sweep_all(a, b, d, r, classes, (f,))[0][f] for a, b, f, r in cases]
    gpu = make()
    for (a, b, f, r), e in zip(cases, exp):
        sr.assert_equal(through_mirror(gpu, a, b, r, f, d), e, f"mirror flags={f} r={r}")
        sr.assert_equal(to_numpy(gpu.query_sweeps(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), r, **kw(f))), e, f"device tensors flags={f} r={r}")
    gpu.close()
    gpu = make()
    gpu.set_host_mirror_limit(0)
    for (a, b, f, r), e in zip(cases, exp):
        sr.assert_equal(gpu.query_sweeps(a, b, r, **kw(f)), e, f"staged kernel flags={f} r={r}")
    assert gpu.frame_stats()["n_host_queries"] == 0
    gpu.close()
    return exp


def one(res, i=0):
    return (int(res["status"][i]), tuple(int(v) for v in res["voxel"][i]), int(res["n_steps"][i]), tuple(int(v) for v in res["hit"][i]),
            int(res["hit_sq"][i]))


# ---- answers written by hand --------------------------------------------------------------------------------------------------
def test_one_obstacle_by_hand_in_all_six_directions(mods):
    """an obstacle 6 voxels along the ray and 3 beside it: radius 3 stops beside it, radius 2 passes; the origin (-4, -3, -5) sends the
    rays through index 0 and through negative blocks"""
    MLMap, _ = mods
    o = np.array([-4, -3, -5])
    E = np.eye(3, dtype=np.int64)
    dirs = [(a, s) for a in range(3) for s in (1, -1)]
    obs = [o + 6 * s * E[a] + 3 * E[(a + 1) % 3] for a, s in dirs]
    b = dump(obs, blocks(-2, 2))
    p0 = centre([o] * 6)
    p1 = centre([o + 12 * s * E[a] for a, s in dirs])
    exp = three_ways(lambda: load(MLMap, b), [(p0, p1, OCC, 3), (p0, p1, OCC, 2), (p0, p1, OCC | INFL | UNKNOWN, 3)], rw.block_classes(b, N))
    for i, (a, s) in enumerate(dirs):
        assert one(exp[0], i) == (1, tuple(o + 6 * s * E[a]), 6, tuple(obs[i]), 9)
        assert one(exp[1], i) == (0, tuple(o + 12 * s * E[a]), 13, tuple(o + 12 * s * E[a]), sr.NONE)
        assert one(exp[2], i) == one(exp[0], i)
    # the plain case of the contract's text
    b = dump([(6, 3, 0)], CUBE3)
    e = three_ways(lambda: load(MLMap, b), [(centre([0, 0, 0]), centre([12, 0, 0]), OCC, 3), (centre([0, 0, 0]), centre([12, 0, 0]), OCC, 2)],
                   rw.block_classes(b, N))
    assert one(e[0]) == (1, (6, 0, 0), 6, (6, 3, 0), 9) and one(e[1])[0] == 0


def test_on_the_sphere_and_just_outside(mods):
    """radius 5: lateral offset (3, 4) stops the ray (25 <= 25), (5, 1) does not (26 > 25), an obstacle dead ahead is met at distance 5"""
    MLMap, _ = mods
    b = dump([(8, 3, 4), (8, 25, 1), (12, 0, 20)], blocks(0, 3))
    p0, p1 = centre([(0, 0, 0), (0, 20, 0), (0, 0, 20)]), centre([(20, 0, 0), (20, 20, 0), (20, 0, 20)])
    exp = three_ways(lambda: load(MLMap, b), [(p0, p1, OCC, 5)], rw.block_classes(b, N))
    assert one(exp[0], 0) == (1, (8, 0, 0), 8, (8, 3, 4), 25)
    assert one(exp[0], 1) == (0, (20, 20, 0), 21, (20, 20, 0), sr.NONE)
    assert one(exp[0], 2) == (1, (7, 0, 20), 7, (12, 0, 20), 25)


def test_ties_go_to_the_smallest_z_then_y_then_x(mods):
    """obstacles that enter the cap in the same step at the same distance and differ in z, in y, in x in turn, and three at once; then
    the same from a ray that starts between them (k = 0: the full ball of the start voxel)"""
    MLMap, _ = mods
    sets = [([(8, 10, 7), (8, 10, 13)], 0, (8, 10, 7)), ([(8, 7, 10), (8, 13, 10)], 0, (8, 7, 10)), ([(7, 8, 10), (13, 8, 10)], 1, (7, 8, 10)),
            ([(8, 10, 13), (8, 13, 10), (8, 7, 10), (8, 10, 7)], 0, (8, 10, 7)), ([(10, 7, 8), (10, 13, 8), (7, 10, 8), (13, 10, 8)], 2, (10, 7, 8))]
    for obs, axis, win in sets:
        b = dump(obs, blocks(0, 2))
        a, e = [10, 10, 10], [10, 10, 10]
        a[axis], e[axis] = 0, 16
        mid = list(a)
        mid[axis] = 8
        p0, p1 = centre([a, mid]), centre([e, e])
        exp = three_ways(lambda: load(MLMap, b), [(p0, p1, OCC, 3), (p0, p1, OCC, 4)], rw.block_classes(b, N))
        assert one(exp[0], 0) == (1, tuple(mid), 8, win, 9) and one(exp[0], 1) == (1, tuple(mid), 0, win, 9)
        assert one(exp[1], 0)[0] == 1 and one(exp[1], 0)[2] == 6 and one(exp[1], 1) == (1, tuple(mid), 0, win, 9)  # (radius 4: met at 2^2 + 3^2 <= 16)


@pytest.mark.parametrize("r", [4, 5, 16])
def test_table_passes_that_do_not_divide_64(mods, r):
    """49, 81 and 797 columns: the only obstacle sits in the table's last column (p, q) = (0, r), whose cap voxel is u_k + r e_c"""
    MLMap, _ = mods
    b = dump([(8, 10, 10 + r), (28, 28, 28)], blocks(0, 3))
    p0, p1 = centre([(0, 10, 10), (0, 10, 9)]), centre([(20, 10, 10), (20, 10, 9)])
    exp = three_ways(lambda: load(MLMap, b), [(p0, p1, OCC, r)], rw.block_classes(b, N))
    assert one(exp[0], 0) == (1, (8, 10, 10), 8, (8, 10, 10 + r), r * r) and one(exp[0], 1)[0] == 0
    assert sr.columns(r) == {4: 49, 5: 81, 16: 797}[r]


# ---- block boundaries and the slot cache ----------------------------------------------------------------------------------------
def test_block_layers_enter_the_slot_cache(mods):
    """a free diagonal ray of 61 voxels through 7 blocks; its only obstacle lies in block (3, 2, 2), which enters the box around the
    ball (radius 6) with the last layer that crosses a block boundary along x"""
    MLMap, _ = mods
    b = dump([(30, 24, 25)], blocks(0, 4))
    p0, p1 = centre([(5, 5, 5), (25, 25, 25), (20, 20, 20)]), centre([(25, 25, 25), (5, 5, 5), (3, 3, 3)])
    exp = three_ways(lambda: load(MLMap, b), [(p0, p1, OCC, 6), (p0, p1, OCC, 5), (p0, p1, OCC | UNKNOWN, 6)], rw.block_classes(b, N))
    assert one(exp[0], 0) == (1, (25, 24, 24), 58, (30, 24, 25), 26) and one(exp[0], 1) == (1, (25, 25, 25), 0, (30, 24, 25), 26)
    assert one(exp[1], 0) == (0, (25, 25, 25), 61, (25, 25, 25), sr.NONE)
    assert one(exp[0], 2)[0] == 0 and one(exp[2], 2) == (1, (5, 6, 6), 43, (-1, 6, 6), 36)  # (absent space beyond the map's edge)


def test_released_and_absent_blocks_and_the_probe_per_lane(mods):
    """subbox_n 5 on a frontier-mode handle: released blocks whose element 0 is 'o', 'f' and 'u' beside a diagonal path (a released
    block's inflated class is UNKNOWN), absent space under MLM_SWEEP_UNKNOWN; radius 2 and 6 keep the block box in the slot cache,
    11 and 16 do not (21 / 5 + 2 = 6 > 5 blocks per axis) and probe per lane"""
    MLMap, _ = mods
    n, d = S5.subbox_n, S5.subbox_d_xyz
    rel = {(4, 1, 1): "o", (1, 4, 1): "f", (1, 1, 4): "u", (5, 5, 2): "o"}
    free = [g for g in blocks(0, 6) if g not in rel and sum(g) % 7 != 3]  # (some blocks absent)
    b = dump([(14, 3, 9), (3, 22, 17)], free, inflated=[(9, 14, 3), (20, 21, 12)], unknown=[(12, 12, 17)], released=rel, n=n)
    classes = rw.block_classes(b, n)
    rng = np.random.default_rng(8)
    v0 = np.concatenate([[(2, 2, 2), (27, 27, 27), (2, 7, 7), (7, 2, 27), (12, 12, 2)], rng.integers(0, 30, size=(27, 3))])
    v1 = np.concatenate([[(27, 27, 27), (2, 2, 2), (27, 7, 7), (7, 27, 2), (12, 12, 29)], rng.integers(0, 30, size=(27, 3))])
    v1[20:] = v0[20:] + rng.integers(-6, 7, size=(12, 3))
    p0, p1 = centre(v0, d), centre(v1, d)
    short = np.array([sr.path_len(x, y, d) <= 30 for x, y in zip(p0, p1)])
    cases = [(p0, p1, f, r) for f in (OCC, UNKNOWN, INFL, OCC | INFL | UNKNOWN) for r in (2, 6, 11)] + [(p0[short], p1[short], OCC, 16), (p0[short], p1[short], INFL, 16)]
    exp = three_ways(lambda: load(MLMap, b, S5), cases, classes, d)
    for e in exp[:3] + exp[-2:]:
        assert (e["status"] == 1).any() and ((e["status"] == 1) & (e["n_steps"] > 0)).any()
    assert (exp[0]["status"] == 0).any() and (exp[6]["status"] == 0).any()


def test_grazing_rays(mods):
    """diagonal rays through exact edges and corners, axis-aligned and zero-length rays (special_rays) over a random map: the ball is
    tested at the grazed voxels too"""
    MLMap, _ = mods
    rng = np.random.default_rng(31)
    b = dump([], blocks(-2, 2))
    b["occ"][rng.random(b["occ"].shape) < 0.01] = ord("o")  # (an obstacle next to most voxels a ray grazes)
    b["infl"][rng.random(b["infl"].shape) < 0.01] = ord("o")
    p0, p1 = rw.special_rays(rng, -2 * N * D, 2 * N * D, D, count=8)
    exp = three_ways(lambda: load(MLMap, b), [(p0, p1, OCC, 1), (p0, p1, OCC | INFL, 2), (p0, p1, OCC, 3)], rw.block_classes(b, N))
    for e in exp:
        assert ((e["status"] == 1) & (e["n_steps"] > 0) & (e["hit_sq"] > 0)).sum() >= 5 and (e["status"] == 0).sum() >= 5, \
            (((e["status"] == 1) & (e["n_steps"] > 0) & (e["hit_sq"] > 0)).sum(), (e["status"] == 0).sum())


# ---- radius 0 is mlm_query_rays ---------------------------------------------------------------------------------------------------
def radius0_equals_cast_rays(gpu, p0, p1):
    import torch

    names = ("status", "voxel", "t", "n_steps", "n_unknown")
    for f in sr.FLAG_SETS:
        ref = gpu.cast_rays(p0, p1, **kw(f))
        got = [gpu.query_sweeps(p0, p1, 0, **kw(f)), to_numpy(gpu.query_sweeps(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), 0, **kw(f)))]
        got += [{k: np.concatenate([gpu.query_sweeps(p0[i:i + 8], p1[i:i + 8], 0, **kw(f))[k] for i in range(0, 64, 8)]) for k in sr.OUTPUTS}]
        for j, g in enumerate(got):
            m = len(g["status"])
            for k in names:
                assert g[k].tobytes() == ref[k][:m].tobytes(), (f, j, k)
            stop = g["status"] == 1
            assert np.array_equal(g["hit"][stop], g["voxel"][stop]) and (g["hit_sq"][stop] == 0).all() and (g["hit_sq"][~stop] == sr.NONE).all()
            assert np.array_equal(g["hit"][~stop], g["voxel"][~stop])
        assert (ref["status"] == -1).any() and ((ref["status"] == 1).any() or f == 0)


def rays_for_radius0(rng, lo, hi):
    u0, u1 = rw.uniform_rays(rng, lo, hi, 300, short=8 * D)
    s0, s1 = rw.special_rays(rng, lo, hi, D, count=40)
    w0, w1 = rw.weird_rays(D)
    return np.ascontiguousarray(np.concatenate([u0, s0, w0])), np.ascontiguousarray(np.concatenate([u1, s1, w1]))


def test_radius_0_equals_query_rays_on_a_random_dump(mods):
    MLMap, _ = mods
    rng = np.random.default_rng(41)
    gpu = load(MLMap, random_dump(rng, N), SX)
    radius0_equals_cast_rays(gpu, *rays_for_radius0(rng, -3 * N * D, 3 * N * D))
    gpu.close()


# ---- the oracle's scene ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(mods):
    """S1, 3 frames of the synthetic room: the library's map and the oracle's block dump"""
    MLMap, OracleMap = mods
    gpu, cpu = MLMap(S1, max_blocks=8192), OracleMap(S1)
    for img, (q, t) in syn.stream(S1, "room_jitter", "smooth", 3):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    b = cpu.export_blocks()
    yield gpu, b
    gpu.close()


def surface_edges(b, rng, count, reach=0.6):
    """edges between points near surfaces: both ends within `reach` metres of an OCCUPIED voxel each, at most ~2 m apart"""
    blk, cid = np.nonzero(b["occ"] == ord("o"))
    assert len(blk) > 100
    vox = b["keys"][blk] * N + np.stack([cid % N, cid // N % N, cid // (N * N)], axis=1)
    i = rng.choice(len(vox), count)
    near = vox[i] + rng.integers(-10, 11, size=(count, 3))
    j = np.array([rng.choice(np.flatnonzero(np.abs(vox - v).max(axis=1) <= 12)) for v in near])
    p0 = vox[i] * D + rng.uniform(-reach, reach, size=(count, 3))
    p1 = vox[j] * D + rng.uniform(-reach, reach, size=(count, 3))
    return np.ascontiguousarray(p0), np.ascontiguousarray(p1)


def test_radius_0_equals_query_rays_on_the_scene(scene):
    gpu, b = scene
    rng = np.random.default_rng(43)
    lo, hi = b["keys"].min(0) * N * D - 0.5, (b["keys"].max(0) + 1) * N * D + 0.5
    radius0_equals_cast_rays(gpu, *rays_for_radius0(rng, lo, hi))


@pytest.mark.parametrize("r", [1, 3, 6])
def test_oracle_scene_and_the_distance_field(scene, r):
    """200 edges between points near surfaces against sweep_ref over the oracle's classes; then mlm_export_esdf at max_dist r + 1 over
    a window that covers the edges: sqdist equals hit_sq at the stop voxel and is greater than r^2 at every earlier path voxel"""
    import torch

    gpu, b = scene
    classes = rw.block_classes(b, N)
    rng = np.random.default_rng(50 + r)
    p0, p1 = surface_edges(b, rng, 200, reach=1.4)
    got = None
    for f in ((OCC, OCC | INFL | UNKNOWN) if r == 3 else (OCC,)):
        exp = sr.sweep_all(p0, p1, D, r, classes, (f,))[0][f]
        dev = to_numpy(gpu.query_sweeps(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), r, **kw(f)))
        sr.assert_equal(dev, exp, f"scene, device flags={f} r={r}")
        sr.assert_equal(gpu.query_sweeps(p0, p1, r, **kw(f)), exp, f"scene, 200 edges in host memory flags={f} r={r}")
        sr.assert_equal(through_mirror(gpu, p0[:24], p1[:24], r, f, D), {k: v[:24] for k, v in exp.items()}, f"scene, mirror flags={f} r={r}")
        got = got or exp
    st = got["status"]
    assert (st == 1).sum() >= 40 and (st == 0).sum() >= 10 and ((st == 1) & (got["n_steps"] > 0) & (got["hit_sq"] > 0)).sum() >= 20, \
        ((st == 1).sum(), (st == 0).sum())
    paths = [[v for v, _ in rw.path(*rw.valid(a, c, D))[0]] for a, c in zip(p0, p1)]
    allv = np.array([v for p in paths for v in p], dtype=np.int64)
    lo = allv.min(axis=0)
    dims = allv.max(axis=0) - lo + 1
    sqd = gpu.export_esdf(lo, dims, r + 1)["sqdist"]
    field = lambda v: int(sqd[v[2] - lo[2], v[1] - lo[1], v[0] - lo[0]])
    for i, p in enumerate(paths):
        k = int(got["n_steps"][i]) if st[i] == 1 else len(p)
        assert all(field(v) > r * r for v in p[:k]), i
        if st[i] == 1:
            assert field(p[k]) == got["hit_sq"][i] and tuple(got["voxel"][i]) == p[k], i


def test_consistent_with_export_reach(scene):
    """a field of mlm_export_reach at clearance r with the same flags, and edges inside its box.  A move of the field (a reached voxel
    and the reached neighbour its parent code names) is never stopped; an edge that stops inside the box stops at a voxel whose steps
    is MLM_REACH_NONE; an edge from a reached voxel that is not stopped and stays in the box runs over reached voxels only (its path is
    6-connected and every voxel of it is traversable)"""
    import torch

    from mlmapping_amd.mlmap import MLM_REACH_NONE

    gpu, b = scene
    r, f = 2, OCC | UNKNOWN
    blk, cid = np.nonzero(b["occ"] == ord("o"))
    mid = np.median(b["keys"][blk] * N + np.stack([cid % N, cid // N % N, cid // (N * N)], axis=1), axis=0).astype(np.int64)
    lo, dims = mid - 20, np.array([40, 40, 40])
    esdf = gpu.export_esdf(lo, dims, r + 1, **kw(f))["sqdist"]
    free = np.argwhere(esdf > r * r)  # (z, y, x)
    assert len(free) > 2000
    seed = free[len(free) // 2][::-1] + lo
    out = gpu.export_reach(lo, dims, [seed], clearance=r, parent=True, **kw(f))
    steps, parent = out["steps"], out["parent"]
    reached = np.argwhere(steps >= 0)
    print(f"free {len(free)}, reached {len(reached)}, not reached {(steps == MLM_REACH_NONE).sum()}")
    assert len(reached) > 1000 and (steps == MLM_REACH_NONE).sum() > 1000
    rng = np.random.default_rng(6)
    pick = reached[rng.choice(len(reached), 400)]
    pick = pick[parent[pick[:, 0], pick[:, 1], pick[:, 2]] < 6]
    moves = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)])
    v = pick[:, ::-1] + lo
    w = v + moves[parent[pick[:, 0], pick[:, 1], pick[:, 2]]]
    g = gpu.query_sweeps(centre(v), centre(w), r, **kw(f))
    print(f"moves {len(v)}, stopped {(g['status'] == 1).sum()}")
    assert len(v) > 300 and (g["status"] == 0).all() and (g["n_steps"] == 2).all()
    # edges between voxels of the box
    a, c = rng.integers(0, 40, size=(300, 3)) + lo, rng.integers(0, 40, size=(300, 3)) + lo
    a[:150] = reached[rng.choice(len(reached), 150)][:, ::-1] + lo
    p0, p1 = centre(a), centre(c)
    g = to_numpy(gpu.query_sweeps(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), r, **kw(f)))
    at_ = lambda x: int(steps[x[2] - lo[2], x[1] - lo[1], x[0] - lo[0]])
    stopped = g["status"] == 1
    print(f"edges stopped {stopped.sum()}, from reached voxels and not stopped {(~stopped[:150]).sum()}")
    assert stopped.sum() >= 50 and (~stopped[:150]).sum() >= 10
    for i in np.flatnonzero(stopped):
        assert at_(g["voxel"][i]) == MLM_REACH_NONE, i
    for i in np.flatnonzero(~stopped[:150]):
        assert all(at_(x) >= 0 for x, _ in rw.path(*rw.valid(p0[i], p1[i], D))[0]), i


# ---- ordering, chunks, arguments ------------------------------------------------------------------------------------------------
def test_async_mode_observes_the_map(mods):
    """after mlm_integrate_depth_batch in async mode, without sync(): the call sees every submitted frame"""
    MLMap, OracleMap = mods
    nf = 4
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(S1, max_blocks=8192, max_batch=4), OracleMap(S1)
    for k in range(nf):
        cpu.update_depth(frames[k], q[k], t[k])
    b = cpu.export_blocks()
    p0, p1 = surface_edges(b, np.random.default_rng(2), 100)
    exp = sr.sweep_all(p0, p1, D, 2, rw.block_classes(b, N), (OCC | UNKNOWN,))[0][OCC | UNKNOWN]
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    sr.assert_equal(gpu.query_sweeps(p0, p1, 2, occ=True, unknown=True), exp, "async")
    gpu.close()


def test_two_chunks_of_host_memory(mods):
    """2^18 + 3 copies of 5 distinct rays in host memory, mirror limit 0: two launches, every copy equals its original"""
    MLMap, _ = mods
    b = dump([(6, 3, 0), (-4, 2, 1)], CUBE3)
    gpu = load(MLMap, b)
    gpu.set_host_mirror_limit(0)
    p0 = np.concatenate([centre([(0, 0, 0), (0, 0, 0), (-4, 2, 0)]), [[np.nan, 0.0, 0.0]], at([(700, -200, 77)])])
    p1 = np.concatenate([centre([(12, 0, 0), (0, 12, 0), (5, 5, 5)]), [[1.0, 1.0, 1.0]], at([(-3000, 4000, 77)])])
    exp = sr.sweep_all(p0, p1, D, 3, rw.block_classes(b, N), (OCC,))[0][OCC]
    assert exp["status"].tolist()[:4] == [1, 0, 1, -1] and exp["n_steps"][2] == 0
    n = SWEEP_CHUNK + 3
    before = gpu.frame_stats()["device_bytes"]
    got = gpu.query_sweeps(np.tile(p0, (n // 5 + 1, 1))[:n], np.tile(p1, (n // 5 + 1, 1))[:n], 3)
    assert gpu.frame_stats()["device_bytes"] - before >= 93 * SWEEP_CHUNK  # (the staging of one chunk is counted)
    assert gpu.frame_stats()["n_host_queries"] == 0
    idx = np.arange(n) % 5
    sr.assert_equal(got, {k: v[idx] for k, v in exp.items()}, "copies")
    gpu.close()


def test_arguments_and_single_outputs(mods, knobs):
    MLMap, _ = mods
    b = dump([(6, 3, 0)], CUBE3)
    for mirror in (1, 0):
        knobs.set("mirror", mirror)
        gpu = load(MLMap, b)
        L, h = gpu._L, gpu._h
        P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        p0 = np.ascontiguousarray(np.concatenate([centre([(0, 0, 0), (0, 1, 0)]), [[np.inf, 0.0, 0.0]]]))
        p1 = np.ascontiguousarray(np.concatenate([centre([(12, 0, 0), (0, 9, 0)]), [[0.0, 0.0, 0.0]]]))
        outs = [np.zeros(3, np.int8), np.zeros((3, 3), np.int32), np.zeros(3, np.float64), np.zeros(3, np.int32), np.zeros(3, np.int32),
                np.zeros((3, 3), np.int32), np.zeros(3, np.int32)]
        call = lambda a=p0, c=p1, n=3, r=3, f=OCC, o=outs: L.mlm_query_sweeps(h, P(a), P(c), n, r, f, *[P(x) for x in o])
        for bad in (lambda: call(n=-1), lambda: call(a=None), lambda: call(c=None), lambda: call(f=8), lambda: call(f=-1), lambda: call(f=OCC | 1 << 20),
                    lambda: call(r=-1), lambda: call(r=17), lambda: call(r=1 << 20), lambda: call(o=[None] * 7)):
            assert bad() == -1
            assert call() == 0  # (the handle is usable afterwards)
        assert call(a=None, c=None, n=0) == 0  # n == 0
        assert call() == 0
        assert outs[0].tolist() == [1, 0, -1] and outs[1].tolist() == [[6, 0, 0], [0, 9, 0], [0, 0, 0]] and outs[3].tolist() == [6, 9, 0]
        assert outs[5].tolist() == [[6, 3, 0], [0, 9, 0], [0, 0, 0]] and outs[6].tolist() == [9, -1, -1] and outs[2][1:].tolist() == [1.0, 0.0]
        full = [o.copy() for o in outs]
        for k in range(7):  # only one output, each in turn
            outs[k][...] = 9
            assert call(o=[outs[j] if j == k else None for j in range(7)]) == 0
            assert np.array_equal(outs[k], full[k]), k
        assert call(f=0, r=16) == 0 and outs[0].tolist() == [0, 0, -1]  # (no class selected: nothing stops a ray)
        assert call(r=0) == 0 and outs[0].tolist() == [0, 0, -1]
        # a batch beyond the mirror's bound is not answered on the host: a ray of 13 voxels at radius 16 is 33^3 + 12 * 797 = 45 501
        # voxels, 8 of them are more than 2^18, 5 are not
        a8, c8, o8 = np.tile(p0[:1], (8, 1)), np.tile(p1[:1], (8, 1)), [np.zeros(8, np.int8)] + [None] * 6
        before = gpu.frame_stats()["n_host_queries"]
        assert call(a=a8, c=c8, n=8, r=16, o=o8) == 0 and gpu.frame_stats()["n_host_queries"] == before and o8[0].tolist() == [1] * 8
        assert call(a=a8, c=c8, n=5, r=16, o=o8) == 0 and gpu.frame_stats()["n_host_queries"] == before + 5 * mirror
        gpu.close()


# ---- the slot cache's bound in small-block geometries ---------------------------------------------------------------------------
BOUNDARY = [(2, 4), (2, 5), (3, 6), (3, 7), (4, 8), (4, 9), (7, 14), (7, 15), (16, 16), (16, 1)]  # (subbox_n, radius): 2 n is the largest cached radius
DB = 0.15


def boundary_rays(n):
    """(start voxel, end voxel) of an axis-parallel and a diagonal ray, each in positive space, in negative space and across voxel 0;
    every one crosses a block boundary"""
    L, m = n + 2, n // 2 + 2
    h = (m + 1) // 2
    return [((1, 1, 1), (1 + L, 1, 1)), ((-2, -2, -2), (-2, -2 - L, -2)), ((0, 1, -L // 2 - 1), (0, 1, L - L // 2)),
            ((1, 1, 1), (1 + m, 1 + m, 1 + m)), ((-2, -2, -2), (-2 - m, -2 - m, -2 - m)), ((-h, h, -h), (-h + m, h - m, -h + m))]


def boundary_map(n):
    """the FREE blocks of a cube wide enough for every ray and the largest ball of this subbox_n, less one absent block (dead ahead of
    the first ray) and with one released block (dead ahead of the second): (free blocks, absent key, released key)"""
    R = max(r for k, r in BOUNDARY if k == n)
    B = -(-(R + n + 6) // n)
    absent, released = ((n + 3) // n, 0, 0), (-1, (-n - 4) // n, -1)
    free = [g for g in blocks(-B, B) if g != absent and g != released]
    return free, absent, released


def place(path, r, n, kind, forbidden):
    """an obstacle voxel for a ray with the path voxels `path` and the path index at which it stops the ray (None: the ray passes), or
    None where the geometry has no such voxel.  exact: at squared distance r^2 of the stop voxel; outside: r^2 + 1 from the nearest
    path voxel; layer: in the block layer that enters the box around the ball at the stop's own step; corner: two blocks away from
    the stop voxel's block on as many axes as the ball allows (the corner of a box of five blocks per axis); sixth_lo / sixth_hi: in
    the first / last block layer of a box that is six blocks wide on some axis (a torus of five would hold both in one cell)"""
    P = np.array(path, dtype=np.int64)
    off, sq = sr.ball(r)
    blk = lambda v: np.floor_divide(v, n)
    ok = lambda c: ~np.array([(blk(c) == np.array(g)).all(axis=-1) for g in forbidden]).any(axis=0)
    clear_before = lambda c, k: ((c[:, None, :] - P[None, :k, :]) ** 2).sum(axis=2).min(axis=1) > r * r  # no path voxel before k within r

    if kind == "outside":
        a = np.arange(-r - 1, r + 2)
        cube = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3) + P[len(P) // 2]
        dist = ((cube[:, None, :] - P[None, :, :]) ** 2).sum(axis=2).min(axis=1)
        cand = cube[(dist == r * r + 1) & ok(cube)]
        return (tuple(int(x) for x in cand[0]), None) if len(cand) else None
    best = None
    for k in range(len(P) - 1, 0, -1):
        step = P[k] - P[k - 1]
        a = int(np.flatnonzero(step)[0])
        s = int(step[a])
        c = P[k] + off
        if kind == "exact":
            c = c[sq == r * r]
        if kind == "exact" and k > 2 * len(P) // 3:
            continue
        c = c[ok(c)]
        if kind != "layer" and len(c):
            c = c[clear_before(c, k)]
        if kind.startswith("sixth"):
            lo_g, hi_g = blk(P[k] - r), blk(P[k] + r)
            for b in np.flatnonzero(hi_g - lo_g == 5):
                cb = c[blk(c)[:, b] == (lo_g if kind == "sixth_lo" else hi_g)[b]] if len(c) else c
                if len(cb):
                    return tuple(int(x) for x in cb[0]), k
        elif kind == "exact":
            if len(c):
                return tuple(int(x) for x in c[0]), k
        elif kind == "layer":
            lead = (P[k][a] + s * r) // n
            if lead != (P[k - 1][a] + s * r) // n:  # (no earlier path voxel reaches this layer)
                c = c[blk(c)[:, a] == lead]
                if len(c):
                    return tuple(int(x) for x in c[-1]), k
        elif kind == "corner" and len(c):
            wide = (blk(P[k] + r) - blk(P[k] - r) == 4) | ((2 * r - 1) // n + 2 > 5)  # (five blocks wide where the box is cached at all)
            score = ((np.abs(blk(c) - blk(P[k])) == 2) & wide).sum(axis=1)
            i = int(np.argmax(score))
            if score[i] >= 1 and (best is None or score[i] > best[2]):
                best = (tuple(int(x) for x in c[i]), k, int(score[i]))
    return best[:2] if best else None


def boundary_scenes(n, r):
    """[(what, block dump, ray index, flags, the path index of the stop or None, the obstacle or None)]"""
    free, absent, released = boundary_map(n)
    rays = boundary_rays(n)
    scenes = []
    for i, (a, b) in enumerate(rays):
        path = [v for v, _ in rw.path(*rw.valid(centre(a, DB)[0], centre(b, DB)[0], DB))[0]]
        for j, kind in enumerate(("layer", "corner", "exact", "outside", "sixth_lo", "sixth_hi")):
            got = place(path, r, n, kind, {absent, released})
            if got is None:
                continue
            o, k = got
            inflated = (i + j) % 2 == 1  # (every other obstacle is an inflated voxel, met with OCC | INFL)
            d = dump([] if inflated else [o], free, inflated=[o] if inflated else (), released={released: b"f"}, n=n)
            # (the scene in full: the ray's voxels, the one obstacle among FREE blocks, where it stops the ray)
            stop = "passes" if k is None else f"stops at path index {k}, voxel {tuple(int(x) for x in path[k])}"
            scenes.append((f"ray {i} {kind} {o}: {'inflated' if inflated else 'OCCUPIED'} voxel {o}, ray from voxel {a} to {b} {stop}, absent block {absent}, "
                           f"released block {released}", d, i, OCC | INFL if inflated else OCC, k, o))
    plain = dump([], free, released={released: b"f"}, n=n)
    scenes += [(f"ray {i} absent block {absent}: ray from voxel {a} to {b}, no obstacle", plain, i, UNKNOWN, None, None) for i, (a, b) in enumerate(rays)]
    solid = dump([], free, released={released: b"o"}, n=n)
    scenes += [(f"ray {i} released block {released}, OCCUPIED: ray from voxel {a} to {b}, no other obstacle", solid, i, OCC, None, None) for i, (a, b) in enumerate(rays)]
    return scenes, rays, absent, released


@pytest.mark.parametrize("n,r", BOUNDARY)
def test_sweep_cache_boundary_geometries(mods, n, r):
    """subbox_n 2, 3, 4 and 7 at the largest radius whose block box stays in the slot cache (2 n: the box is exactly five blocks wide,
    an entering layer takes the torus cells of the leaving one) and at the next one (probed per lane), 16 at radius 16 and 1.  One
    obstacle per scene — in the block layer that enters at the step of the stop, in the corner block of the box, on the sphere, just
    outside it, and at radius 2 n + 1 in the first and in the last layer of a box six blocks wide — for six rays; then no obstacle at
    all: the absent block under UNKNOWN, and the released block once it is OCCUPIED.  Every scene is imported into the same two
    handles in turn: mirror and device tensors on one, the staged kernel on the other.  A failure names its scene in full (ray,
    obstacle, stop, subbox_n, radius): dump([obstacle], boundary_map(n)[0], n=n) and one query_sweeps reproduce it."""
    import torch

    MLMap, _ = mods
    cfg = SX.with_(subbox_n=n, subbox_d_xyz=DB)
    scenes, rays, absent, released = boundary_scenes(n, r)
    p0, p1 = centre([a for a, _ in rays], DB), centre([b for _, b in rays], DB)
    exp, kinds = [], set()
    for what, b, i, f, k, o in scenes:
        e = sr.sweep_all(p0[i:i + 1], p1[i:i + 1], DB, r, rw.block_classes(b, n), (f,))[0][f]
        exp.append(e)
        if o is not None and k is not None:
            assert one(e)[0] == 1 and one(e)[2] == k and one(e)[3] == o, (what, one(e))
            kinds.add(what.split()[2])
        elif o is not None:
            assert one(e)[0] == 0, (what, one(e))
            kinds.add("outside")
    assert {"layer", "exact", "outside"} <= kinds and ("corner" in kinds) == (2 * n <= r + 1), kinds  # (a block two away lies in the ball from r = 2 n - 1 on)
    assert ({"sixth_lo", "sixth_hi"} <= kinds) == (r == 2 * n + 1) and (r == 2 * n + 1 or not {"sixth_lo", "sixth_hi"} & kinds), kinds
    in_block = lambda e, g: one(e)[0] == 1 and tuple(np.floor_divide(one(e)[3], n).tolist()) == g
    assert in_block(exp[-12], absent) and in_block(exp[-5], released), (one(exp[-12]), one(exp[-5]))  # (the first ray, the second ray)
    zeros = np.zeros(scenes[0][1]["occ"].shape, np.float32)
    for staged in (False, True):
        gpu = load(MLMap, scenes[0][1], cfg)
        if staged:
            gpu.set_host_mirror_limit(0)
        for (what, b, i, f, k, o), e in zip(scenes, exp):
            gpu.import_blocks(b["keys"], zeros, b["occ"], b["infl"], b["collapsed"])
            a, c = np.ascontiguousarray(p0[i:i + 1]), np.ascontiguousarray(p1[i:i + 1])
            if staged:
                sr.assert_equal(gpu.query_sweeps(a, c, r, **kw(f)), e, f"staged kernel n={n} r={r} {what}")
            else:
                sr.assert_equal(through_mirror(gpu, a, c, r, f, DB), e, f"mirror n={n} r={r} {what}")
                sr.assert_equal(to_numpy(gpu.query_sweeps(torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda(), r, **kw(f))), e, f"device tensors n={n} r={r} {what}")
        assert staged == (gpu.frame_stats()["n_host_queries"] == 0)
        gpu.close()
