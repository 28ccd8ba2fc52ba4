"""mlm_query_rays: batched segment casts through the voxel map (include/mlmap_hip.h), every output held exactly (t by its 64 bits)
to the walk of the header's contract written in plain Python integers (tests/raywalk_ref.py) over classes that do not come from the
code under test: maps built voxel by voxel, and the CPU oracle's block dumps and point queries.  The kernel (k_rays) and the host
mirror must give the same bytes."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import raywalk_ref as rw

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN
D, N = S1.subbox_d_xyz, S1.subbox_n


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def cast(gpu, p0, p1, flags):
    return gpu.cast_rays(p0, p1, occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN))


def same_bytes(a, b, what=""):
    for k in rw.OUTPUTS:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def window_classes(gpu, lo, dims):
    """classes(voxels) inside a box from the GPU's own export_window"""
    w = gpu.export_window(lo, dims, odds=False, occ=True, infl=True)
    occ, infl = w["occ"].astype(np.int64), w["infl"].astype(np.int64)
    bits = np.where(occ == 0, OCC, np.where(occ == -1, UNKNOWN, 0)) | np.where(infl == 0, INFL, 0)
    return bits


# ---- maps built voxel by voxel ------------------------------------------------------------------------------------------------
def crafted(MLMap, obstacles, free_blocks, inflated=()):
    """obstacle voxels OCCUPIED (and `inflated` voxels inflated-OCCUPIED) in otherwise FREE blocks; everything else UNKNOWN"""
    obs = np.asarray(obstacles, dtype=np.int64).reshape(-1, 3)
    inf = np.asarray(inflated, dtype=np.int64).reshape(-1, 3)
    keys = np.unique(np.concatenate([np.floor_divide(obs, N), np.floor_divide(inf, N), np.asarray(free_blocks, dtype=np.int64).reshape(-1, 3)]), axis=0)
    occ = np.full((len(keys), N ** 3), ord("f"), dtype=np.uint8)
    infl = np.full((len(keys), N ** 3), ord("u"), dtype=np.uint8)
    kidx = {tuple(k): i for i, k in enumerate(keys.tolist())}
    for arr, plane in ((obs, occ), (inf, infl)):
        for v in arr:
            g = np.floor_divide(v, N)
            c = v - g * N
            plane[kidx[tuple(g.tolist())], (c[2] * N + c[1]) * N + c[0]] = ord("o")
    b = {"keys": keys.astype(np.int32), "occ": occ, "infl": infl, "collapsed": np.zeros(len(keys), np.uint8)}
    gpu = MLMap(S1, max_blocks=4096)
    gpu.import_blocks(b["keys"], np.zeros(occ.shape, np.float32), occ, infl, b["collapsed"])
    return gpu, b


def test_crafted_maps_by_hand(mods):
    """single obstacle voxels, a plane with a one-voxel gap, negative coordinates: stop voxel, t and counts written by hand"""
    MLMap, _ = mods
    plane = [(7, y, z) for y in range(-12, 13) for z in range(-6, 7) if (y, z) != (2, 1)]  # the plane x = 7 with a gap at y 2, z 1
    free = [(gx, gy, gz) for gx in range(-2, 2) for gy in range(-2, 2) for gz in range(-1, 1)]  # voxels -20 .. 19, -20 .. 19, -10 .. 9
    gpu, b = crafted(MLMap, plane + [(-13, -4, -3), (3, 3, 3)], free, inflated=[(5, -7, 0), (-13, -4, -2)])
    c = lambda *v: [(x + 0.5 + 0.25 / 1024) * D for x in v]  # a voxel's centre, a quarter lattice unit up: lattice coordinate 1024 x + 512
    # (p0, p1, flags) -> (status, voxel, t, n_steps, n_unknown); rays along +x from x = 0.5 voxels: voxel k is entered at
    # m / |D| = (1024 k - 512) / |D| lattice units
    L = 14 * 1024  # lattice length of the rays from voxel 0 to voxel 14 along x
    hand = [
        (c(0, 0, 0), c(14, 0, 0), OCC, (1, (7, 0, 0), (7 * 1024 - 512) / L, 7, 0)),          # stops at the plane
        (c(0, 2, 1), c(14, 2, 1), OCC, (0, (14, 2, 1), 1.0, 15, 0)),                         # through the gap
        (c(0, 2, 1), c(24, 2, 1), OCC, (0, (24, 2, 1), 1.0, 25, 5)),                         # ... and on into unknown space (x >= 20)
        (c(0, 2, 1), c(24, 2, 1), UNKNOWN, (1, (20, 2, 1), (20 * 1024 - 512) / (24 * 1024), 20, 0)),
        (c(0, 2, 1), c(24, 2, 1), 0, (0, (24, 2, 1), 1.0, 25, 5)),                           # a pure count
        (c(0, -7, 0), c(14, -7, 0), OCC | INFL, (1, (5, -7, 0), (5 * 1024 - 512) / L, 5, 0)),  # the inflated voxel in front of the plane
        (c(0, -7, 0), c(14, -7, 0), OCC, (1, (7, -7, 0), (7 * 1024 - 512) / L, 7, 0)),
        (c(14, 0, 0), c(0, 0, 0), OCC, (1, (7, 0, 0), (7 * 1024 - 512) / L, 7, 0)),            # from the other side: voxel 7 after 7 steps too
        (c(-13, -4, 5), c(-13, -4, -9), OCC, (1, (-13, -4, -3), (8 * 1024 - 512) / L, 8, 0)),  # down -z at negative coordinates
        (c(-13, -4, 5), c(-13, -4, -9), INFL, (1, (-13, -4, -2), (7 * 1024 - 512) / L, 7, 0)),
        (c(3, 3, 3), c(9, 9, 9), OCC, (1, (3, 3, 3), 0.0, 0, 0)),                            # starts inside an obstacle
        (c(0, 0, 0), c(0, 0, 0), OCC, (0, (0, 0, 0), 1.0, 1, 0)),                            # zero length
        (c(-25, 0, 0), c(-15, 0, 0), OCC, (0, (-15, 0, 0), 1.0, 11, 5)),                     # out of unknown space: x -25 .. -21 unknown
        # the exact diagonal through voxel corners from the corner (0,0,0): ties go x, then y, then z; (1,0,0) and (1,1,0) are grazed
        ([0.0, 0.0, 0.0], [3 * D, 3 * D, 3 * D], OCC, None),
    ]
    classes = rw.block_classes(b, N)
    lo, dims = [-30, -30, -15], [60, 60, 30]
    iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
    vox = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1)
    assert np.array_equal(classes(vox), window_classes(gpu, lo, dims).reshape(-1))  # (the test's classes are the GPU's window classes)
    for i, (a, e, flags, want) in enumerate(hand):
        got = cast(gpu, [a], [e], flags)
        exp, _ = rw.cast(np.array(a), np.array(e), D, classes, (flags,))
        if want is not None:
            assert exp[flags] == want, (i, exp[flags], want)  # (the hand-written answer and the Python walk agree)
        g = (int(got["status"][0]), tuple(int(v) for v in got["voxel"][0]), float(got["t"][0]), int(got["n_steps"][0]), int(got["n_unknown"][0]))
        assert g == exp[flags], (i, g, exp[flags])
    got = cast(gpu, [[0.0, 0.0, 0.0]], [[3 * D, 3 * D, 3 * D]], 0)
    assert got["n_steps"][0] == 10 and tuple(got["voxel"][0]) == (3, 3, 3)
    # the rest by the walk: rays through the crafted region, the special end points, every flag set
    rng = np.random.default_rng(2)
    r0, r1 = rw.uniform_rays(rng, [-2.6, -2.6, -1.3], [2.6, 2.6, 1.3], 1500, short=0.8)
    s0, s1 = rw.special_rays(rng, np.array([-2.6, -2.6, -1.3]), np.array([2.6, 2.6, 1.3]), D, count=100)
    q0, q1 = np.concatenate([r0, s0]), np.concatenate([r1, s1])
    exp, ties = rw.cast_all(q0, q1, D, classes)
    assert (ties > 0).sum() >= 50
    for f in rw.FLAG_SETS:
        rw.assert_equal(cast(gpu, q0, q1, f), exp[f], f"crafted flags={f}")
    gpu.close()


# ---- real maps ----------------------------------------------------------------------------------------------------------------
def real_map(mods, frontier):
    MLMap, OracleMap = mods
    if frontier:
        cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
        gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=2), OracleMap(cfg)
        for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 8):
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
    else:
        cfg = S1
        gpu, cpu = MLMap(cfg, max_blocks=8192), OracleMap(cfg)
        for k, (img, (q, t)) in enumerate(syn.stream(cfg, "room_jitter", "smooth", 6)):
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
            if k in (2, 4):
                gpu.inflate_map(t)
                cpu.inflate_map(t)
    return cfg, gpu, cpu


def map_rays(b, cfg, seed, count, n_special=60):
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    rng = np.random.default_rng(seed)
    lo, hi = b["keys"].min(0) * d * n - 1.0, (b["keys"].max(0) + 1) * d * n + 1.0
    parts = [rw.uniform_rays(rng, lo, hi, count, short=1.5), rw.special_rays(rng, lo, hi, d, count=n_special), rw.weird_rays(d)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


N_REAL = 20000


@pytest.mark.parametrize("frontier", [False, True], ids=["S1", "S1 frontier n5"])
def test_real_maps_against_the_oracle(mods, knobs, frontier):
    """20 000 rays per flag set (and the special and invalid ones) over the oracle's classes; the first 3 000 again on a handle
    whose kernel runs with three workgroups (many rays per lane)"""
    cfg, gpu, cpu = real_map(mods, frontier)
    b = cpu.export_blocks()
    if frontier:
        assert b["collapsed"].sum() > 20
    classes = rw.block_classes(b, cfg.subbox_n)
    rng = np.random.default_rng(4)
    lo_v, hi_v = b["keys"].min(0) * cfg.subbox_n - 10, (b["keys"].max(0) + 1) * cfg.subbox_n + 10
    vox = rng.integers(lo_v, hi_v, size=(20000, 3))  # the block dump's classes are the oracle's point queries at the centres
    assert np.array_equal(classes(vox), rw.query_classes(cpu.getOccupancy, cpu.getInflateOccupancy, cfg)(vox))
    p0, p1 = map_rays(b, cfg, 6, N_REAL)
    exp, ties = rw.cast_all(p0, p1, cfg.subbox_d_xyz, classes)
    rw.non_vacuous(exp, ties, N_REAL)
    for f in rw.FLAG_SETS:
        rw.assert_equal(cast(gpu, p0, p1, f), exp[f], f"frontier={frontier} flags={f}")
    gpu.close()
    knobs.set("rays_grid", 3)
    knobs.set("mirror", 0)
    cfg, gpu, _ = real_map(mods, frontier)
    for f in rw.FLAG_SETS:
        rw.assert_equal(cast(gpu, p0[:3000], p1[:3000], f), {k: v[:3000] for k, v in exp[f].items()}, f"three workgroups frontier={frontier} flags={f}")
    gpu.close()


def test_mirror_and_kernel_give_the_same_bytes(mods, knobs):
    """one batch through the host mirror (small batches, default knobs), through the kernel (mirror = 0), and split into batches of
    1, 7, 64, 65 and 4 097 rays"""
    cfg, gpu, cpu = real_map(mods, False)
    p0, p1 = map_rays(cpu.export_blocks(), cfg, 9, 6000, n_special=20)
    n = len(p0)
    for f in (OCC | INFL, OCC, UNKNOWN):
        ref = cast(gpu, p0, p1, f)
        before = gpu.frame_stats()["n_host_queries"]
        for size in (1, 7, 64, 65, 4097):
            parts = [cast(gpu, p0[i:i + size], p1[i:i + size], f) for i in range(0, n if size > 7 else 300 * size, size)]
            m = sum(len(p["status"]) for p in parts)
            same_bytes({k: np.concatenate([p[k] for p in parts]) for k in rw.OUTPUTS}, {k: ref[k][:m] for k in rw.OUTPUTS}, (f, size))
        assert gpu.frame_stats()["n_host_queries"] > before  # (the small batches were answered on the host)
    keep = cast(gpu, p0, p1, OCC | INFL)
    gpu.close()
    knobs.set("mirror", 0)  # every batch through the kernel
    cfg, gpu2, _ = real_map(mods, False)
    same_bytes(cast(gpu2, p0, p1, OCC | INFL), keep, "kernel, whole batch")
    for size in (1, 7, 64):
        parts = [cast(gpu2, p0[i:i + size], p1[i:i + size], OCC | INFL) for i in range(0, 60 * size, size)]
        m = 60 * size
        same_bytes({k: np.concatenate([p[k] for p in parts]) for k in rw.OUTPUTS}, {k: keep[k][:m] for k in rw.OUTPUTS}, ("kernel", size))
    assert gpu2.frame_stats()["n_host_queries"] == 0
    gpu2.close()


def test_a_million_rays_in_one_call(mods):
    """2^20 rays of 0 to 2 000 voxels: a 5 000-ray sample against the walk; the same rays in shuffled order give the same answers"""
    cfg, gpu, cpu = real_map(mods, False)
    b = cpu.export_blocks()
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    rng = np.random.default_rng(12)
    cnt = 1 << 20
    lo, hi = b["keys"].min(0) * d * n - 1.0, (b["keys"].max(0) + 1) * d * n + 1.0
    p0 = rng.uniform(lo, hi, size=(cnt, 3))
    u = rng.normal(size=(cnt, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p1 = p0 + u * (rng.uniform(0.0, 1.0, size=(cnt, 1)) ** 2 * 2000.0 * d)
    p1[::1000] = p0[::1000]  # zero length
    got = cast(gpu, p0, p1, 0)
    assert got["n_steps"].max() > 1500 and (got["n_steps"] == 1).sum() >= cnt // 1000
    classes = rw.block_classes(b, n)
    pick = rng.choice(cnt, 5000, replace=False)
    for f in (0, OCC):
        g = got if f == 0 else cast(gpu, p0, p1, f)
        exp, _ = rw.cast_all(p0[pick], p1[pick], d, classes, (f,))
        rw.assert_equal({k: g[k][pick] for k in rw.OUTPUTS}, exp[f], f"2^20 flags={f}")
        perm = rng.permutation(cnt)
        sh = cast(gpu, p0[perm], p1[perm], f)
        same_bytes({k: sh[k][np.argsort(perm)] for k in rw.OUTPUTS}, g, f"shuffled flags={f}")
    gpu.close()


# ---- destinations, modes, arguments ------------------------------------------------------------------------------------------
def test_async_stream_and_device_memory(mods):
    """async mode without sync(): the rays see every submitted frame; device inputs and outputs on the caller's stream, behind
    queued work, give the host result; the staging grows at most at the first call and then stays"""
    import torch

    MLMap, OracleMap = mods
    nf = 8
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(S1, max_blocks=8192, max_batch=4), OracleMap(S1)
    for k in range(nf):
        cpu.update_depth(frames[k], q[k], t[k])
    b = cpu.export_blocks()
    p0, p1 = map_rays(b, S1, 3, 5000, n_special=10)
    exp, _ = rw.cast_all(p0, p1, D, rw.block_classes(b, N), (OCC | INFL,))
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    before = gpu.frame_stats()["device_bytes"]
    w = cast(gpu, p0, p1, OCC | INFL)
    rw.assert_equal(w, exp[OCC | INFL], "async")
    grown = gpu.frame_stats()["device_bytes"]
    assert grown >= before
    cast(gpu, p0, p1, OCC)
    assert gpu.frame_stats()["device_bytes"] == grown

    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    n = len(p0)
    dev = {"status": torch.empty(n, dtype=torch.int8, device="cuda"), "voxel": torch.empty((n, 3), dtype=torch.int32, device="cuda"),
           "t": torch.empty(n, dtype=torch.float64, device="cuda"), "n_steps": torch.empty(n, dtype=torch.int32, device="cuda"),
           "n_unknown": torch.empty(n, dtype=torch.int32, device="cuda")}
    junk = torch.ones(1 << 26, device="cuda")
    h0, h1 = torch.from_numpy(p0).pin_memory(), torch.from_numpy(p1).pin_memory()
    with torch.cuda.stream(s):
        for _ in range(50):  # (keeps the caller's stream busy: the end points arrive, and the answers are written, behind this work)
            junk.mul_(1.0001)
        d0, d1 = h0.to("cuda", non_blocking=True), h1.to("cuda", non_blocking=True)
        for v in dev.values():
            v.fill_(7)
    gpu.cast_rays_dev(d0.data_ptr(), d1.data_ptr(), n, occ=True, infl=True, **{k: v.data_ptr() for k, v in dev.items()})
    same_bytes({k: v.cpu().numpy() for k, v in dev.items()}, w, "device")
    # device inputs, host outputs
    out = np.empty(n, dtype=np.int32)
    assert gpu._L.mlm_query_rays(gpu._h, ctypes.c_void_p(d0.data_ptr()), ctypes.c_void_p(d1.data_ptr()), n, OCC | INFL, None, None, None,
                                 out.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert np.array_equal(out, w["n_steps"])
    assert gpu.frame_stats()["device_bytes"] == grown
    gpu.close()


def test_arguments_null_outputs_invalid_rays_and_empty_map(mods, knobs):
    MLMap, _ = mods
    for mirror in (1, 0):
        knobs.set("mirror", mirror)
        gpu = MLMap(S1, max_blocks=1024)
        L, h = gpu._L, gpu._h
        vp = ctypes.c_void_p
        a = np.array([[0.05 * D, 0.5 * D, 0.5 * D], [np.nan, 0, 0], [0.5 * D, 0.5 * D, 0.5 * D]])
        e = np.array([[3.5 * D, 0.5 * D, 0.5 * D], [1, 1, 1], [0.5 * D, 2.5 * D, 0.5 * D]])
        pa, pe = a.ctypes.data_as(vp), e.ctypes.data_as(vp)
        outs = [np.zeros(3, np.int8), np.zeros((3, 3), np.int32), np.zeros(3, np.float64), np.zeros(3, np.int32), np.zeros(3, np.int32)]
        po = [o.ctypes.data_as(vp) for o in outs]
        ok = lambda: L.mlm_query_rays(h, pa, pe, 3, OCC, *po)
        # each refused argument, the handle usable afterwards
        for bad in (lambda: L.mlm_query_rays(h, pa, pe, -1, OCC, *po), lambda: L.mlm_query_rays(h, None, pe, 3, OCC, *po),
                    lambda: L.mlm_query_rays(h, pa, None, 3, OCC, *po), lambda: L.mlm_query_rays(h, pa, pe, 3, 8, *po),
                    lambda: L.mlm_query_rays(h, pa, pe, 3, -1, *po), lambda: L.mlm_query_rays(h, pa, pe, 3, OCC | 1 << 20, *po),
                    lambda: L.mlm_query_rays(h, pa, pe, 3, OCC, None, None, None, None, None)):
            assert bad() == -1
            assert ok() == 0
        assert L.mlm_query_rays(h, None, None, 0, OCC, *po) == 0  # n == 0
        # an empty map: OCC never stops and counts every voxel as unknown; UNKNOWN stops at path index 0; the invalid ray between
        # two valid ones is -1 / zeros and leaves its neighbours alone
        assert ok() == 0
        assert outs[0].tolist() == [0, -1, 0] and outs[3].tolist() == [4, 0, 3] and outs[4].tolist() == [4, 0, 3]
        assert outs[1].tolist() == [[3, 0, 0], [0, 0, 0], [0, 2, 0]] and outs[2].tolist() == [1.0, 0.0, 1.0]
        assert L.mlm_query_rays(h, pa, pe, 3, UNKNOWN, *po) == 0
        assert outs[0].tolist() == [1, -1, 1] and outs[3].tolist() == [0, 0, 0] and outs[4].tolist() == [0, 0, 0] and outs[2].tolist() == [0.0, 0.0, 0.0]
        assert outs[1].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
        # every combination of one output
        full = [o.copy() for o in outs]
        for k in range(5):
            outs[k][...] = 9
            one = [po[j] if j == k else None for j in range(5)]
            assert L.mlm_query_rays(h, pa, pe, 3, UNKNOWN, *one) == 0
            assert np.array_equal(outs[k], full[k]), k
        gpu.close()


def test_answers_follow_the_map(mods):
    """after setFree_map_in_bound and after a further update_map the (mirror's and the kernel's) answers follow the map"""
    cfg, gpu, cpu = real_map(mods, False)
    frames = list(syn.stream(cfg, "room_jitter", "smooth", 8))
    p0, p1 = map_rays(cpu.export_blocks(), cfg, 21, 4000, n_special=10)
    small = slice(0, 40)

    def check(what):
        classes = rw.block_classes(cpu.export_blocks(), cfg.subbox_n)
        exp, _ = rw.cast_all(p0, p1, cfg.subbox_d_xyz, classes, (OCC, UNKNOWN))
        for f in (OCC, UNKNOWN):
            rw.assert_equal(cast(gpu, p0[small], p1[small], f), {k: v[small] for k, v in exp[f].items()}, f"{what} mirror flags={f}")
            rw.assert_equal(cast(gpu, p0, p1, f), exp[f], f"{what} kernel flags={f}")
        return exp

    first = check("start")
    b = cpu.export_blocks()
    dg = cfg.subbox_d_xyz * cfg.subbox_n
    mid = (b["keys"].min(0) + b["keys"].max(0) + 1) * 0.5 * dg
    gpu.setFree_map_in_bound(mid - 1.2, mid + 1.2)
    cpu.setFree_map_in_bound(mid - 1.2, mid + 1.2)
    second = check("setFree")
    assert not np.array_equal(first[OCC]["n_steps"], second[OCC]["n_steps"])
    for img, (q, t) in frames[6:]:
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    third = check("update")
    assert not np.array_equal(second[OCC]["n_steps"], third[OCC]["n_steps"])
    gpu.close()
