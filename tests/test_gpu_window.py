"""mlm_export_window: a dense box of voxels read out in one call — odds, occupancy, inflate occupancy and odds gradients at every
voxel, which must be what the per-position queries return there (float / double bits, equal int8 classes) and agree with the CPU
oracle bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import assert_same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _halo() -> int:
    with open(os.path.join(ROOT, "mlmapping_amd", "csrc", "mlm_kernels_window.h")) as f:
        return int(re.search(r"#define MLM_WIN_HALO (\d+)", f.read()).group(1))


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


@pytest.fixture(scope="module")
def s1_maps(mods):
    """S1 after six room_jitter frames, on the GPU and in the oracle"""
    MLMap, OracleMap = mods
    gpu, cpu = MLMap(S1, max_blocks=8192), OracleMap(S1)
    for img, (q, t) in syn.stream(S1, "room_jitter", "smooth", 6):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    yield gpu, cpu
    gpu.close()


def window_voxels(cfg, lo, dims, sel=None):
    """Block keys [N,3], cell ids [N] and centres [N,3] of the window's voxels in its (dz, dy, dx) order (sel: those flat indices
    only); centres as tests/util.py::voxel_centres computes them (subbox_id2xyz_glb_vec, map_local.h:208-213)."""
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    idx = np.arange(dims[0] * dims[1] * dims[2]) if sel is None else sel
    iz, iy, ix = np.unravel_index(idx, (dims[2], dims[1], dims[0]))
    v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
    keys = np.floor_divide(v, n)
    cc = v - keys * n
    cid = cc[:, 2] * n * n + cc[:, 1] * n + cc[:, 0]
    cen = keys.astype(np.float64) * (d * n) + cc.astype(np.float64) * d + d * 0.5
    return keys.astype(np.int32), cid.astype(np.int32), cen


def map_window(b, cfg):
    """A window that is not block aligned, not a multiple of subbox_n, and covers every allocated block with one block of margin"""
    n = cfg.subbox_n
    lo = b["keys"].min(0) * n - 7
    hi = (b["keys"].max(0) + 2) * n - 4
    return [int(v) for v in lo], [int(v) for v in hi - lo]


def check_queries(gpu, w, keys, cid, cen, max_iter, sel=None):
    """every channel of w bit for bit what the per-position queries return at the voxels (sel: the flat indices of w that keys /
    cid / cen describe)"""
    flat = {k: (v.reshape(-1, 3) if k == "grad" else v.reshape(-1)) for k, v in w.items()}
    if sel is not None:
        flat = {k: v[sel] for k, v in flat.items()}
    if "odds" in flat:
        assert np.array_equal(flat["odds"].view(np.uint32), gpu.getOddAt(keys, cid).view(np.uint32)), "odds differ from getOdd"
    if "occ" in flat:
        assert np.array_equal(flat["occ"].astype(np.int32), gpu.getOccupancy(cen)), "occ differs from getOccupancy"
    if "infl" in flat:
        assert np.array_equal(flat["infl"].astype(np.int32), gpu.getInflateOccupancy(cen)), "infl differs from getInflateOccupancy"
    if "grad" in flat:
        gq = gpu.getOddGrad(cen, max_iter)
        bad = np.flatnonzero((flat["grad"].view(np.uint64) != gq.view(np.uint64)).any(axis=1))
        assert bad.size == 0, f"{bad.size} gradients differ from getOddGrad, first at {cen[bad[0]]}: {flat['grad'][bad[0]]} vs {gq[bad[0]]}"


def check_oracle(cpu, w, keys, cid, cen, max_iter, sel=None):
    flat = {k: (v.reshape(-1, 3) if k == "grad" else v.reshape(-1)) for k, v in w.items()}
    if sel is not None:
        flat = {k: v[sel] for k, v in flat.items()}
    if "odds" in flat:
        assert_same_bits(flat["odds"], cpu.getOddAt(keys, cid), "window odds vs the oracle")
    if "occ" in flat:
        assert np.array_equal(flat["occ"].astype(np.int32), cpu.getOccupancy(cen))
    if "infl" in flat:
        assert np.array_equal(flat["infl"].astype(np.int32), cpu.getInflateOccupancy(cen))
    if "grad" in flat:
        assert_same_bits(flat["grad"], cpu.getOddGrad(cen, max_iter), "window gradients vs the oracle")


ALL = dict(odds=True, occ=True, infl=True, grad=True)


@pytest.mark.parametrize("max_iter", [0, 1, 5, "beyond halo"])
def test_window_matches_queries_and_oracle(s1_maps, max_iter):
    """S1, a window around the whole map (absent blocks and negative indices included): every channel equals the queries and agrees
    with the oracle; max_iter 0 gives zero gradients, a max_iter beyond the halo takes the lookups past it."""
    gpu, cpu = s1_maps
    if max_iter == "beyond halo":
        max_iter = _halo() + 3
    b = cpu.export_blocks()
    lo, dims = map_window(b, S1)
    assert min(lo) < 0 and all(d % S1.subbox_n for d in dims) and all(v % S1.subbox_n for v in lo)
    w = gpu.export_window(lo, dims, max_iter=max_iter, **ALL)
    assert w["odds"].shape == (dims[2], dims[1], dims[0]) and w["grad"].shape == (dims[2], dims[1], dims[0], 3)
    keys, cid, cen = window_voxels(S1, lo, dims)
    check_queries(gpu, w, keys, cid, cen, max_iter)
    check_oracle(cpu, w, keys, cid, cen, max_iter)
    assert (w["occ"] == 0).any() and (w["occ"] == 1).any() and (w["occ"] == -1).any()
    if max_iter == 0:
        assert not w["grad"].any()
    else:
        assert w["grad"].any()


def test_one_voxel_thick_slice(s1_maps):
    """dims[2] == 1 at a height through the scene: the shape of the visualize_odds slice (src/mlmap.cpp:200-284)"""
    gpu, cpu = s1_maps
    b = cpu.export_blocks()
    lo, dims = map_window(b, S1)
    lo[2], dims[2] = 12, 1
    w = gpu.export_window(lo, dims, max_iter=5, **ALL)
    assert w["odds"].shape == (1, dims[1], dims[0])
    keys, cid, cen = window_voxels(S1, lo, dims)
    check_queries(gpu, w, keys, cid, cen, 5)
    check_oracle(cpu, w, keys, cid, cen, 5)
    assert (w["occ"] == 0).any() and (w["occ"] == 1).any()


def test_frontier_mode_released_blocks(mods):
    """use_exploration_frontiers: released blocks (vectors of size 1, map_local.cpp:208-232) answer from element 0 — odds, occ and
    every gradient step into them — and are UNKNOWN for infl"""
    MLMap, OracleMap = mods
    cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
    gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=2), OracleMap(cfg)
    frames = list(syn.stream(cfg, "room_jitter", "smooth", 8))
    for k, (img, (q, t)) in enumerate(frames):
        if k % 5 == 3:  # a two-frame synchronous batch in between
            continue
        if k % 5 == 4:
            fr = frames[k - 1:k + 1]
            gpu.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
            for f in fr:
                cpu.update_depth(f[0], *f[1])
        else:
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
    b = cpu.export_blocks()
    assert b["collapsed"].sum() > 20
    lo, dims = map_window(b, cfg)
    w = gpu.export_window(lo, dims, max_iter=5, **ALL)
    keys, cid, cen = window_voxels(cfg, lo, dims)
    check_queries(gpu, w, keys, cid, cen, 5)
    check_oracle(cpu, w, keys, cid, cen, 5)
    col = {tuple(k) for k in b["keys"][b["collapsed"].astype(bool)]}
    in_col = np.array([tuple(k) in col for k in map(tuple, keys)])
    assert in_col.sum() >= 20 * cfg.cells_per_block
    assert (w["infl"].reshape(-1)[in_col] == -1).all()
    gpu.close()


def test_infl_after_inflate_map(mods):
    """after inflate_map (src/mlmap.cpp:286-309) the infl channel holds inflated cells, as getInflateOccupancy and the oracle do"""
    MLMap, OracleMap = mods
    gpu, cpu = MLMap(S1, max_blocks=8192), OracleMap(S1)
    for k, (img, (q, t)) in enumerate(syn.stream(S1, "room_jitter", "smooth", 5)):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
        if k in (2, 4):
            gpu.inflate_map(t)
            cpu.inflate_map(t)
    b = cpu.export_blocks()
    lo, dims = map_window(b, S1)
    w = gpu.export_window(lo, dims, odds=False, infl=True)
    assert list(w) == ["infl"] and (w["infl"] == 0).sum() > 100
    keys, cid, cen = window_voxels(S1, lo, dims)
    check_queries(gpu, w, keys, cid, cen, 5)
    check_oracle(cpu, w, keys, cid, cen, 5)
    gpu.close()


def test_async_mode_and_caller_stream(mods):
    """async mode: a window read right after an asynchronous submission sees every submitted frame; with the caller's torch
    stream and device tensors as destinations the result is the host-destination result"""
    import torch

    MLMap, OracleMap = mods
    n = 8
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", n)])
    poses = syn.smooth_trajectory(n, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(S1, max_blocks=8192, max_batch=4), OracleMap(S1)
    for k in range(n):
        cpu.update_depth(frames[k], q[k], t[k])
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    b = cpu.export_blocks()
    lo, dims = map_window(b, S1)
    w = gpu.export_window(lo, dims, max_iter=5, **ALL)
    keys, cid, cen = window_voxels(S1, lo, dims)
    check_oracle(cpu, w, keys, cid, cen, 5)

    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    shape = (dims[2], dims[1], dims[0])
    dev = {"odds": torch.empty(shape, dtype=torch.float32, device="cuda"), "occ": torch.empty(shape, dtype=torch.int8, device="cuda"),
           "infl": torch.empty(shape, dtype=torch.int8, device="cuda"), "grad": torch.empty(shape + (3,), dtype=torch.float64, device="cuda")}
    junk = torch.ones(1 << 26, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(50):  # (keeps the caller's stream busy: the window is written behind this work)
            junk.mul_(1.0001)
        for v in dev.values():
            v.fill_(7)
    gpu.export_window_dev(lo, dims, 5, **{k: v.data_ptr() for k, v in dev.items()})
    host = gpu.export_window(lo, dims, max_iter=5, **ALL)
    for k, v in dev.items():
        a = v.cpu().numpy()
        assert np.array_equal(a.view(np.uint8), host[k].view(np.uint8)), f"{k}: device destination differs from host destination"
        assert np.array_equal(a.view(np.uint8), w[k].view(np.uint8)), k
    gpu.close()


def test_large_window(s1_maps):
    """a 512 x 512 x 64 window (16.7 M voxels: several tiles, bricks per block row, grid-stride loops) against the queries at
    500 k voxels drawn at random"""
    gpu, cpu = s1_maps
    lo, dims = [-250, -240, -20], [512, 512, 64]
    w = gpu.export_window(lo, dims, odds=True, occ=True, grad=True, max_iter=5)
    sel = np.random.default_rng(5).choice(dims[0] * dims[1] * dims[2], 500000, replace=False)
    keys, cid, cen = window_voxels(S1, lo, dims, sel)
    check_queries(gpu, w, keys, cid, cen, 5, sel)
    assert (w["occ"] == 0).sum() > 1000


def test_empty_map(mods):
    """no frames: odds 0.5, occ and infl UNKNOWN, zero gradients; the gradient scratch is kept by the handle and counted"""
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=1024)
    before = gpu.frame_stats()["device_bytes"]
    lo, dims = [-13, -5, -9], [37, 23, 11]
    w = gpu.export_window(lo, dims, max_iter=5, **ALL)
    assert (w["odds"] == 0.5).all() and (w["occ"] == -1).all() and (w["infl"] == -1).all() and not w["grad"].any()
    grown = gpu.frame_stats()["device_bytes"]
    assert grown > before
    gpu.export_window(lo, dims, max_iter=5, **ALL)
    assert gpu.frame_stats()["device_bytes"] == grown
    gpu.close()


def test_invalid_arguments(mods):
    """each refused argument gives MLM_ERR_INVALID and leaves the handle usable"""
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=1024)
    L, h = gpu._L, gpu._h
    buf = np.zeros(1 << 16, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)

    def call(lo, dims, max_iter=5, outs=(p, None, None, None)):
        lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
        return L.mlm_export_window(h, lo_a.ctypes.data_as(ctypes.c_void_p), dims_a.ctypes.data_as(ctypes.c_void_p), max_iter, *outs)

    cases = [([0, 0, 0], [0, 4, 4]), ([0, 0, 0], [4, -1, 4]), ([0, 0, 0], [4, 4, 0]),
             ([0, 0, 0], [2048, 2048, 1024]), ([0, 0, 0], [65536, 32768, 1]),
             ([2 ** 31 - 10, 0, 0], [20, 1, 1]), ([0, 0, 2 ** 31 - 1], [1, 1, 1])]
    for lo, dims in cases:
        assert call(lo, dims) == -1, (lo, dims)
        assert call([0, 0, 0], [4, 4, 4]) == 0
    assert call([0, 0, 0], [4, 4, 4], max_iter=-1) == -1
    assert call([0, 0, 0], [4, 4, 4], outs=(None, None, None, None)) == -1
    assert call([0, 0, 0], [4, 4, 4], outs=(None, None, None, p)) == 0
    assert (buf[:192] == 0).all()  # (an empty map: zero gradients)
    w = gpu.export_window([2 ** 31 - 11, -2 ** 31, 0], [10, 3, 2], occ=True, grad=True)  # the int32 extremes: absent blocks
    assert (w["odds"] == 0.5).all() and (w["occ"] == -1).all() and not w["grad"].any()
    gpu.close()
