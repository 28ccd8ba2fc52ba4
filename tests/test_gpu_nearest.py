"""mlm_query_nearest: the exact nearest obstacle voxel of batched points (include/mlmap_hip.h), every output held byte for byte to the
contract written in plain Python integers (tests/nearest_ref.py: every voxel of the cube, no pruning) over classes that do not come
from the code under test: maps built voxel by voxel, and the CPU oracle's block dump.  Every case runs three ways — small batches in
host memory (the host mirror), device tensors for every pointer (the kernel k_nearest), and host memory again after
set_host_mirror_limit(0) (the kernel, staged) — and all three must give the same bytes.  (The mirror takes a batch only while
n * (2C + 1)^3 <= 2^18: from C = 32 on no batch qualifies and that leg asserts that nothing was answered on the host.)

The cross-check with mlm_export_esdf reads `status == 0 where sqdist == C^2` as: no obstacle nearer than C.  An obstacle at a distance
of exactly C voxels lies inside the ball (E == (1024 C)^2) and is reported, while the clamped sqdist is C^2 either way; there the
test asks for sq == C^2 * 2^20, and the reference decides which of the two holds."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import nearest_ref as nr
from tests import raywalk_ref as rw

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN = nr.OCC, nr.INFL, nr.UNKNOWN
D, N = S1.subbox_d_xyz, S1.subbox_n
SX = S1.with_(use_exploration_frontiers=True)  # released blocks answer from element 0 only in frontier mode
NEAR_CHUNK = 1 << 18     # points per launch when host memory is staged (include/mlmap_hip.h: "65 bytes x 2^18 points")
MIRROR_VOXELS = 1 << 18  # the mirror's bound on n * (2C + 1)^3


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def dump(obstacles, free_blocks, inflated=(), unknown=(), released=None, n=N):
    """obstacle voxels OCCUPIED, `unknown` voxels UNKNOWN and `inflated` voxels inflated-OCCUPIED in otherwise FREE blocks; `released`
    {block: b'o' / b'f' / b'u'}: released blocks with that element 0; everything else absent"""
    released = released or {}
    arrs = [np.asarray(a, dtype=np.int64).reshape(-1, 3) for a in (obstacles, inflated, unknown)]
    keys = np.unique(np.concatenate([np.floor_divide(a, n) for a in arrs] + [np.asarray(list(free_blocks) + list(released), dtype=np.int64).reshape(-1, 3)]), axis=0)
    occ = np.full((len(keys), n ** 3), ord("f"), dtype=np.uint8)
    infl = np.full((len(keys), n ** 3), ord("u"), dtype=np.uint8)
    col = np.zeros(len(keys), np.uint8)
    kidx = {tuple(k): i for i, k in enumerate(keys.tolist())}
    for arr, plane, ch in ((arrs[0], occ, "o"), (arrs[1], infl, "o"), (arrs[2], occ, "u")):
        for v in arr:
            g = np.floor_divide(v, n)
            c = v - g * n
            plane[kidx[tuple(g.tolist())], (c[2] * n + c[1]) * n + c[0]] = ord(ch)
    for g, ch in released.items():
        col[kidx[tuple(g)]] = 1
        occ[kidx[tuple(g)], 0] = ord(ch)
    return {"keys": keys.astype(np.int32), "occ": occ, "infl": infl, "collapsed": col}


def load(MLMap, b, cfg=S1):
    gpu = MLMap(cfg, max_blocks=4096)
    gpu.import_blocks(b["keys"], np.zeros(b["occ"].shape, np.float32), b["occ"], b["infl"], b["collapsed"])
    return gpu


def at(Q, d=D):
    """positions whose lattice coordinates are exactly Q (integers, 1024 per voxel; 1024 v + 512 is the centre of voxel v)"""
    Q = np.asarray(Q, dtype=np.int64).reshape(-1, 3)
    p = (Q + 0.5) * d / 1024.0
    assert all(rw.lattice(x, d) == q for x, q in zip(p, Q.tolist()))
    return p


def centre(v, d=D):
    return at(np.asarray(v, dtype=np.int64).reshape(-1, 3) * 1024 + 512, d)


def kw(flags):
    return {"occ": bool(flags & OCC), "infl": bool(flags & INFL), "unknown": bool(flags & UNKNOWN)}


def to_numpy(out):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in out.items()}


def through_mirror(gpu, pts, flags, C):
    """the batch in host memory in pieces the mirror takes (at most 8 points at first: the mirror needs a refresh; then 64), or, where
    no piece qualifies, nothing: returns the answers or None"""
    side = (2 * C + 1) ** 3
    if side > MIRROR_VOXELS:
        before = gpu.frame_stats()["n_host_queries"]
        gpu.query_nearest(pts[:1], C, **kw(flags))
        assert gpu.frame_stats()["n_host_queries"] == before, "a batch beyond the mirror's bound was answered on the host"
        return None
    parts, i = [], 0
    while i < len(pts):
        m = min(8 if i == 0 else 64, MIRROR_VOXELS // side, len(pts) - i)
        before = gpu.frame_stats()["n_host_queries"]
        parts.append(gpu.query_nearest(pts[i:i + m], C, **kw(flags)))
        assert gpu.frame_stats()["n_host_queries"] == before + m, "the batch was not answered by the host mirror"
        i += m
    return {k: np.concatenate([p[k] for p in parts]) for k in nr.OUTPUTS}


def three_ways(make, cases, classes, d=D):
    """cases: [(points, flags, C)] on the map make() builds: mirror and device tensors on one handle, then the kernel with staged host
    memory on a handle after set_host_mirror_limit(0); everything equal to nearest_ref.  Returns the reference's answers."""
    import torch

    exp = [nr.nearest_all(p, d, C, classes, f)[0] for p, f, C in cases]
    gpu = make()
    for (p, f, C), e in zip(cases, exp):
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
        g = through_mirror(gpu, p, f, C)
        if g is not None:
            nr.assert_equal(g, e, f"mirror flags={f} C={C}")
        nr.assert_equal(to_numpy(gpu.query_nearest(torch.from_numpy(p).cuda(), C, **kw(f))), e, f"device tensors flags={f} C={C}")
    gpu.close()
    gpu = make()
    gpu.set_host_mirror_limit(0)
    for (p, f, C), e in zip(cases, exp):
        nr.assert_equal(gpu.query_nearest(np.asarray(p, dtype=np.float64), C, **kw(f)), e, f"staged kernel flags={f} C={C}")
    assert gpu.frame_stats()["n_host_queries"] == 0
    gpu.close()
    return exp


def one(res, i=0):
    return (int(res["status"][i]), tuple(int(v) for v in res["voxel"][i]), tuple(int(v) for v in res["delta"][i]), int(res["sq"][i]),
            float(res["dist"][i]))


CUBE3 = [(gx, gy, gz) for gx in (-1, 0, 1) for gy in (-1, 0, 1) for gz in (-1, 0, 1)]  # voxels -10 .. 19 on every axis


# ---- answers written by hand --------------------------------------------------------------------------------------------------
def test_one_obstacle_by_hand(mods):
    MLMap, _ = mods
    b = dump([(3, 0, 0)], CUBE3)
    p = centre([0, 0, 0])
    exp = three_ways(lambda: load(MLMap, b), [(p, OCC, 3), (p, OCC, 2), (p, OCC | INFL | UNKNOWN, 3)], rw.block_classes(b, N))
    assert one(exp[0]) == (1, (3, 0, 0), (3072, 0, 0), 9 << 20, (float(np.float32(D)) * float(np.sqrt(np.float64(9 << 20)))) / 1024.0)
    assert one(exp[1]) == (0, (0, 0, 0), (0, 0, 0), -1, -1.0)
    assert one(exp[2])[:2] == (1, (3, 0, 0))


def test_ties_go_to_the_smallest_z_then_y_then_x(mods):
    """points on voxel centres between two obstacles at equal E that differ in z, in y and in x in turn; points on voxel faces, edges
    and corners in UNKNOWN space (the tie goes to v - 1 on that axis)"""
    MLMap, _ = mods
    obs = [(2, 2, 0), (2, 2, 4), (12, 0, 2), (12, 4, 2), (0, 12, 2), (4, 12, 2),      # pairs along z, y, x around (2,2,2), (12,2,2), (2,12,2)
           (-5, -5, -3), (-5, -3, -5), (-3, -5, -5), (-5, -5, -7), (-5, -7, -5), (-7, -5, -5)]  # all six neighbours at distance 2 of (-5,-5,-5)
    b = dump(obs, CUBE3)
    classes = rw.block_classes(b, N)
    pts = centre([(2, 2, 2), (12, 2, 2), (2, 12, 2), (-5, -5, -5)])
    faces = at([(1024 * 30, 1024 * 30 + 512, 1024 * 30 + 512), (1024 * 30, 1024 * 30, 1024 * 30 + 100), (1024 * 30, 1024 * 30, 1024 * 30),
                (-1024 * 40, 1024 * 30 + 512, -1024 * 40)])  # in absent space
    exp = three_ways(lambda: load(MLMap, b), [(pts, OCC, 3), (pts, OCC | INFL, 6), (faces, UNKNOWN, 2), (faces, OCC | UNKNOWN, 5)], classes)
    assert [one(exp[0], i)[1] for i in range(4)] == [(2, 2, 0), (12, 0, 2), (0, 12, 2), (-5, -5, -7)]
    assert [one(exp[2], i)[1] for i in range(4)] == [(29, 30, 30), (29, 29, 30), (29, 29, 29), (-41, 30, -41)]
    assert one(exp[2], 2)[3] == 3 * 512 * 512


def test_block_boundaries_and_rings(mods):
    """an obstacle in a diagonal block of ring 2 nearer than one in ring 1 (a ring loop that stops one ring early answers the other);
    an obstacle in a ring-1 block whose bound EQUALS the best E of ring 0 and which wins by the tie rule alone (pruning with >= loses it)"""
    MLMap, _ = mods
    big = [(gx, gy, gz) for gx in range(-3, 5) for gy in range(-3, 5) for gz in (-1, 0, 1)]
    b1 = dump([(20, 20, 9), (-8, 9, 9)], big)
    e1 = three_ways(lambda: load(MLMap, b1), [(centre([9, 9, 9]), OCC, 20), (centre([9, 9, 9]), OCC, 15)], rw.block_classes(b1, N))
    assert one(e1[0])[:2] == (1, (20, 20, 9)) and one(e1[0])[3] == 242 << 20
    assert one(e1[1])[0] == 0  # (|(11, 11, 0)|^2 = 242 > 225, |(-17, 0, 0)|^2 = 289)
    b2 = dump([(5, 5, 5), (-1, 5, 5), (2, 8, 5), (2, 5, 8)], CUBE3)
    e2 = three_ways(lambda: load(MLMap, b2), [(centre([2, 5, 5]), OCC, 3), (centre([2, 5, 5]), OCC, 9)], rw.block_classes(b2, N))
    assert one(e2[0])[:2] == (1, (-1, 5, 5)) and one(e2[1])[:2] == (1, (-1, 5, 5))


def test_absent_and_released_blocks(mods):
    """UNKNOWN selected: a point in mapped free space next to absent space; points inside and beside released blocks whose element 0
    is 'o', 'f' and 'u' (a released block has one class for all its voxels, its inflated class is UNKNOWN)"""
    MLMap, _ = mods
    rel = {(2, 0, 0): "o", (0, 2, 0): "f", (0, 0, 2): "u"}
    b = dump([(5, 5, 5)], [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], inflated=[(7, 7, 7)], released=rel)
    classes = rw.block_classes(b, N)
    pts = np.concatenate([centre([(1, 5, 5), (25, 5, 5), (5, 25, 5), (5, 5, 25), (18, 5, 5), (5, 18, 5), (5, 5, 18), (8, 8, 8)]),
                          at([(1024 * 19 + 1000, 1024 * 5 + 3, 1024 * 5 + 700), (1024 * 5 + 1, 1024 * 5 + 1, 1024 * 19 + 1023)])])
    cases = [(pts, f, C) for f in (OCC, UNKNOWN, OCC | UNKNOWN, INFL, OCC | INFL | UNKNOWN) for C in (2, 7)]
    exp = three_ways(lambda: load(MLMap, b, SX), cases, classes)
    # (cases: flags OCC, UNKNOWN, OCC | UNKNOWN, INFL, all three, each at C = 2 and 7)
    assert one(exp[0], 0)[:2] == (0, (1, 5, 5)) and one(exp[2], 0)[:2] == (1, (-1, 5, 5))        # UNKNOWN: absent space two voxels away
    assert one(exp[0], 1)[:2] == (1, (25, 5, 5)) and one(exp[0], 1)[3] == 0                      # inside the 'o' block: its own voxel
    assert one(exp[0], 4)[:2] == (1, (20, 5, 5)) and one(exp[2], 4)[0] == 0                      # beside the 'o' block: its first layer
    assert one(exp[2], 2)[0] == 0 and one(exp[3], 2)[:2] == (1, (10, 25, 5))                     # 'f': on to absent space, ties to z, then y
    assert one(exp[2], 3)[:2] == (1, (5, 5, 25)) and one(exp[2], 6)[:2] == (1, (5, 5, 20))      # 'u': its own voxel, and from beside it
    assert one(exp[6], 7)[:2] == (1, (7, 7, 7)) and one(exp[6], 1)[0] == 0                      # INFL: never a released block


def test_lane_stepping_over_parts_that_do_not_divide_64(mods):
    """the part of a block inside the cube with extents (1, 1, 3), (3, 7, 2) and the full 10^3, the obstacle in its last cells"""
    MLMap, _ = mods
    # C = 1, the point near the upper x, y corner of voxel (9, 9, 5): block (1, 1, 0) is cut to x 10, y 10, z 4 .. 6
    b1 = dump([(10, 10, 5), (10, 10, 6)], CUBE3)  # ((10, 10, 6) lies in the cube, outside the ball)
    p1 = at([(1024 * 9 + 1000, 1024 * 9 + 1000, 1024 * 5 + 512)])
    e1 = three_ways(lambda: load(MLMap, b1), [(p1, OCC, 1)], rw.block_classes(b1, N))
    assert one(e1[0])[:3] == (1, (10, 10, 5), (536, 536, 0))
    # C = 3, voxel (9, 3, 7): block (1, 0, 1) is cut to x 10 .. 12, y 0 .. 6, z 10 .. 11 (3 x 7 x 2 = 42 cells); its last cell in the ball
    b2 = dump([(10, 5, 10), (10, 1, 10), (11, 3, 11)], CUBE3)
    e2 = three_ways(lambda: load(MLMap, b2), [(centre([9, 3, 7]), OCC, 3), (centre([9, 3, 8]), OCC, 3)], rw.block_classes(b2, N))
    assert one(e2[0])[0] == 0 and one(e2[1])[:2] == (1, (10, 1, 10))  # ((1, 2, 3) is outside the ball, (1, -2, 2) and (1, 2, 2) tie at 9)
    # C = 12, voxel (5, 5, 5): block (0, 0, 0) lies inside the cube whole (1000 cells, 16 steps of 64); the only obstacle in its last cell
    b3 = dump([(9, 9, 9)], CUBE3)
    e3 = three_ways(lambda: load(MLMap, b3), [(centre([5, 5, 5]), OCC, 12), (centre([[5, 5, 5], [0, 0, 0], [9, 0, 9]]), OCC | INFL, 16)], rw.block_classes(b3, N))
    assert one(e3[0])[:2] == (1, (9, 9, 9)) and one(e3[1], 1)[3] == 243 << 20


# ---- random maps ----------------------------------------------------------------------------------------------------------------
def random_dump(rng, n, nblk=40, span=3):
    keys = np.unique(rng.integers(-span, span, size=(nblk, 3)), axis=0).astype(np.int32)
    c = n ** 3
    r = rng.random((len(keys), c))
    occ = np.where(r < 0.004, ord("o"), np.where(r < 0.01, ord("u"), ord("f"))).astype(np.uint8)
    infl = np.where(rng.random((len(keys), c)) < 0.004, ord("o"), ord("u")).astype(np.uint8)
    col = (rng.random(len(keys)) < 0.15).astype(np.uint8)
    occ[col.astype(bool), 0] = rng.choice([ord("f"), ord("f"), ord("u"), ord("o")], size=int(col.sum()))
    return {"keys": keys, "occ": occ, "infl": infl, "collapsed": col}


def random_points(rng, n, d, count):
    lo, hi = -3 * n - 4, 3 * n + 4
    uni = rng.uniform(lo * d, hi * d, size=(count - 96, 3))
    cen = centre(rng.integers(lo, hi, size=(48, 3)), d)
    k = rng.integers(lo, hi, size=(40, 3)) * 1024 + np.where(rng.random((40, 3)) < 0.4, 512, 0)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e300, 0, 0], [0, 0, -1e300], [2.0 ** 40 * d / 1024.0, 0, 0], [0, -(2.0 ** 40 + 2) * d / 1024.0, 0],
                    [5000000 * d, 0.5 * d, 0.5 * d], [0.3 * d, -5000000 * d, 5000000 * d]])
    return np.concatenate([uni, cen, at(k, d), bad])


@pytest.mark.parametrize("which", [0, 1], ids=["n10", "n5 with released blocks"])
def test_random_maps_against_the_brute_force_reference(mods, which):
    MLMap, _ = mods
    cfg = S1 if which == 0 else SX.with_(subbox_n=5)
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    rng = np.random.default_rng(21 + which)
    b = random_dump(rng, n)
    if which == 0:
        b["collapsed"][:] = 0
    classes = rw.block_classes(b, n)
    pts = random_points(rng, n, d, 256)
    cases = [(pts, f, C) for f in nr.FLAG_SETS for C in (1, 4, 9)]
    exp = three_ways(lambda: load(MLMap, b, cfg), cases, classes, d)
    st = np.concatenate([e["status"] for e in exp])
    assert all((st == s).sum() >= 50 for s in (-1, 0, 1)), [(st == s).sum() for s in (-1, 0, 1)]


def test_max_dist_64_in_a_30_block_map(mods):
    """8 points, OCC only: cheap, absent blocks are skipped whole (2 197 block probes per point at most, 30 scans)"""
    MLMap, _ = mods
    rng = np.random.default_rng(5)
    b = random_dump(rng, N, nblk=30, span=4)
    b["collapsed"][:] = 0
    b["occ"][b["occ"] == ord("o")] = ord("f")
    far = [(0, 1, 2), (3, 700, 41), (17, 999, 5)]  # a handful of obstacles: most points find theirs tens of voxels away
    for blk, cell, _ in far:
        b["occ"][blk, cell] = ord("o")
    pts = np.concatenate([rng.uniform(-45 * D, 45 * D, size=(6, 3)), centre([(0, 0, 0), (-90, 60, 10)])])
    exp = three_ways(lambda: load(MLMap, b), [(pts, OCC, 64)], rw.block_classes(b, N))
    assert (exp[0]["status"] == 1).sum() >= 4 and exp[0]["sq"].max() > (30 * 1024) ** 2


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


def test_oracle_scene(mods, scene):
    import torch

    gpu, b = scene
    classes = rw.block_classes(b, N)
    rng = np.random.default_rng(17)
    blk, cid = np.nonzero(b["occ"] == ord("o"))
    assert len(blk) > 100
    pick = rng.choice(len(blk), 150)
    surf = (b["keys"][blk[pick]] * N + np.stack([cid[pick] % N, cid[pick] // N % N, cid[pick] // (N * N)], axis=1)) * D
    pts = np.concatenate([surf + rng.uniform(-1.0, 1.0, size=surf.shape), rng.uniform(b["keys"].min(0) * N * D - 1.0, (b["keys"].max(0) + 1) * N * D + 1.0, size=(50, 3))])
    for f, C in ((OCC, 6), (OCC | INFL | UNKNOWN, 3), (UNKNOWN, 8)):
        exp, _ = nr.nearest_all(pts, D, C, classes, f)
        assert (exp["status"] == 1).sum() >= 40 and (exp["status"] == 0).sum() >= (20 if f == OCC else 0)
        g = through_mirror(gpu, pts[:40], f, C)
        nr.assert_equal(g, {k: v[:40] for k, v in exp.items()}, f"scene, mirror flags={f}")
        nr.assert_equal(to_numpy(gpu.query_nearest(torch.from_numpy(pts).cuda(), C, **kw(f))), exp, f"scene, device flags={f}")
        nr.assert_equal(gpu.query_nearest(pts, C, **kw(f)), exp, f"scene, 200 points in host memory flags={f}")


def test_cross_check_with_export_esdf(mods, scene):
    """a 24^3 window of the scene, C = 6, the voxel centres whose lattice remainder is 512 on all three axes: sq == 2^20 * sqdist
    wherever sqdist < 36; where sqdist == 36 there is no obstacle nearer than 6: status 0, or an obstacle at exactly 6 (sq == 36 * 2^20)"""
    import torch

    gpu, b = scene
    C = 6
    blk, cid = np.nonzero(b["occ"] == ord("o"))
    mid = np.median(b["keys"][blk] * N + np.stack([cid % N, cid // N % N, cid // (N * N)], axis=1), axis=0).astype(np.int64)
    lo = mid - 12
    sqd = gpu.export_esdf(lo, [24, 24, 24], C)["sqdist"].reshape(-1).astype(np.int64)
    z, y, x = np.meshgrid(np.arange(24), np.arange(24), np.arange(24), indexing="ij")
    vox = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) + lo
    pts = (vox + 0.5) * D
    keep = np.array([Q is not None and all(q % 1024 == 512 for q in Q) and [q >> 10 for q in Q] == v for p, v in zip(pts, vox.tolist()) for Q in [rw.lattice(p, D)]])
    assert keep.mean() >= 0.70, keep.mean()  # (92.5 % per axis, about 79 % of triples: the filter cannot hide a failure)
    got = to_numpy(gpu.query_nearest(torch.from_numpy(np.ascontiguousarray(pts[keep])).cuda(), C, outputs=("status", "sq")))
    s, st = sqd[keep], got["status"]
    assert (s < 36).sum() > 500 and (s == 36).sum() > 500
    assert np.array_equal(st[s < 36], np.ones((s < 36).sum(), np.int8)) and np.array_equal(got["sq"][s < 36], s[s < 36] << 20)
    far = s == 36
    assert np.all((st[far] == 0) | ((st[far] == 1) & (got["sq"][far] == 36 << 20)))
    exp, _ = nr.nearest_all(pts[keep][far], D, C, rw.block_classes(b, N), OCC)  # which of the two, for every far point: the reference
    assert np.array_equal(st[far], exp["status"]) and np.array_equal(got["sq"][far], exp["sq"])


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
    rng = np.random.default_rng(2)
    pts = rng.uniform(b["keys"].min(0) * N * D, (b["keys"].max(0) + 1) * N * D, size=(100, 3))
    exp, _ = nr.nearest_all(pts, D, 5, rw.block_classes(b, N), OCC | UNKNOWN)
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    nr.assert_equal(gpu.query_nearest(pts, 5, occ=True, unknown=True), exp, "async")
    gpu.close()


# ---- chunks -------------------------------------------------------------------------------------------------------------------
def test_two_chunks_of_host_memory(mods):
    """2^18 + 3 copies of 5 distinct points in host memory, mirror limit 0: two launches, every copy equals its original"""
    MLMap, _ = mods
    b = dump([(3, 0, 0), (-4, 2, 1)], CUBE3)
    gpu = load(MLMap, b)
    gpu.set_host_mirror_limit(0)
    five = np.concatenate([centre([(0, 0, 0), (-3, 3, 0)]), at([(700, -200, 77)]), [[np.nan, 0.0, 0.0]], centre([(15, 15, 15)])])
    exp, _ = nr.nearest_all(five, D, 3, rw.block_classes(b, N), OCC)
    assert exp["status"].tolist() == [1, 1, 1, -1, 0]
    n = NEAR_CHUNK + 3
    before = gpu.frame_stats()["device_bytes"]
    got = gpu.query_nearest(np.tile(five, (n // 5 + 1, 1))[:n], 3)
    assert gpu.frame_stats()["device_bytes"] - before >= 65 * NEAR_CHUNK  # (the staging of one chunk is counted)
    assert gpu.frame_stats()["n_host_queries"] == 0
    idx = np.arange(n) % 5
    nr.assert_equal(got, {k: v[idx] for k, v in exp.items()}, "copies")
    gpu.close()


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_arguments_and_single_outputs(mods, knobs):
    MLMap, _ = mods
    b = dump([(3, 0, 0)], CUBE3)
    for mirror in (1, 0):
        knobs.set("mirror", mirror)
        gpu = load(MLMap, b)
        L, h = gpu._L, gpu._h
        P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        pts = np.ascontiguousarray(np.concatenate([centre([(0, 0, 0), (0, 3, 0)]), [[np.inf, 0.0, 0.0]]]))
        outs = [np.zeros(3, np.int8), np.zeros((3, 3), np.int32), np.zeros((3, 3), np.int32), np.zeros(3, np.int64), np.zeros(3, np.float64)]
        call = lambda p=pts, n=3, c=3, f=OCC, o=outs: L.mlm_query_nearest(h, P(p), n, c, f, *[P(x) for x in o])
        for bad in (lambda: call(n=-1), lambda: call(p=None), lambda: call(f=0), lambda: call(f=8), lambda: call(f=-1), lambda: call(f=OCC | 1 << 20),
                    lambda: call(c=0), lambda: call(c=65), lambda: call(c=-3), lambda: call(o=[None] * 5)):
            assert bad() == -1
            assert call() == 0  # (the handle is usable afterwards)
        assert call(p=None, n=0) == 0  # n == 0
        assert call() == 0
        assert outs[0].tolist() == [1, 0, -1] and outs[1].tolist() == [[3, 0, 0], [0, 3, 0], [0, 0, 0]]
        assert outs[2].tolist() == [[3072, 0, 0], [0, 0, 0], [0, 0, 0]] and outs[3].tolist() == [9 << 20, -1, -1] and outs[4][1:].tolist() == [-1.0, -1.0]
        full = [o.copy() for o in outs]
        for k in range(5):  # only one output, each in turn
            outs[k][...] = 9
            assert call(o=[outs[j] if j == k else None for j in range(5)]) == 0
            assert np.array_equal(outs[k], full[k]), k
        assert call(c=64, f=OCC | INFL | UNKNOWN) == 0 and outs[0].tolist() == [1, 1, -1]
        gpu.close()


# ---- blocks with fewer cells than a wave has lanes ------------------------------------------------------------------------------
def small_block_maps(n, C):
    """two maps around the point voxel (1, 1, 1): A with OCCUPIED voxels C away along y and inflated ones C away along x (ties within
    a plane and across them), B with OCCUPIED voxels C away along z, one just outside the ball and, far from these, one in the first
    cell of the block diagonally behind the upper corner of block (far(n, C) / n, far(n, C) / n, 0)"""
    W = -(-(min(C, 10) + 2) // n)
    free = [(gx, gy, gz) for gx in range(-W, W + 1) for gy in range(-W, W + 1) for gz in range(-W, W + 1)]
    a = dump([(1, 1 + C, 1), (1, 1 - C, 1)], free, inflated=[(1 + C, 1, 1), (1 - C, 1, 1)], n=n)
    S = far(n, C)
    b = dump([(1, 1, 1 + C), (1, 1, 1 - C), (1 + C, 2, 1), (S + n, S + n, 0)], free + [(S // n, S // n, 0)], n=n)
    return a, b


def far(n, C):
    """a multiple of subbox_n more than 6 C voxels away"""
    return n * (-(-(6 * C + 8) // n))


@pytest.mark.parametrize("C", [1, "n", "n + 1", 17])
@pytest.mark.parametrize("n", [2, 3, 7, 16])
def test_nearest_small_blocks(mods, n, C):
    """subbox_n 2, 3 (a whole block has 8 and 27 cells), 7 and 16 at max_dist 1, n, n + 1 and 17, voxel size 0.15: the winner lies
    C / n block rings out, at a distance of exactly C voxels; two voxels at that distance in different blocks tie and z, then y, then x
    decides; the parts of the blocks at the cube's faces have fewer than 64 cells; a point far from everything finds nothing"""
    MLMap, _ = mods
    C = {"n": n, "n + 1": n + 1}.get(C, C)
    d = 0.15
    cfg = S1.with_(subbox_n=n, subbox_d_xyz=d)
    a, b = small_block_maps(n, C)
    S = far(n, C)
    pts = np.concatenate([centre([(1, 1, 1)], d), at([(1024, 1024 + 512, 1024 + 512), (1024, 1024, 1024)], d),  # a centre, a face, a corner
                          centre([(1, 4 * C + 4, 1)], d), at([(1024 * (S + n - 1) + 1000, 1024 * (S + n - 1) + 1000, 512)], d)])
    ea = three_ways(lambda: load(MLMap, a, cfg), [(pts, OCC, C), (pts, INFL, C), (pts, OCC | INFL, C)], rw.block_classes(a, n), d)
    win = (1, (1, 1 - C, 1), (0, -1024 * C, 0), C * C << 20)
    assert one(ea[0])[:4] == win and one(ea[2])[:4] == win             # y decides between (1, 1 - C, 1) and (1, 1 + C, 1), and before x
    assert one(ea[1])[:4] == (1, (1 - C, 1, 1), (-1024 * C, 0, 0), C * C << 20)  # x decides
    assert [one(e, 3)[0] for e in ea] == [0, 0, 0]                     # nothing in range
    eb = three_ways(lambda: load(MLMap, b, cfg), [(pts, OCC, C), (pts, OCC | UNKNOWN, C)], rw.block_classes(b, n), d)
    assert one(eb[0])[:4] == (1, (1, 1, 1 - C), (0, 0, -1024 * C), C * C << 20)  # z decides; (1 + C, 2, 1) is outside the ball
    assert one(eb[0], 4)[:3] == (1, (S + n, S + n, 0), (536, 536, 0))    # the first cell of its block, a part of one to four cells at C 1
