"""Padded depth images: row_stride > width and frame_stride > row_stride * height on all four depth entry points
(include/mlmap_hip.h), on both Stage A paths, with and without the single-frame graph, and in frontier mode.

The padding columns and the gaps between frames hold random NON-ZERO depths drawn from a seeded generator — every one of them
would be a valid measurement, so a kernel that reads a single padding pixel as image changes the map — and the oracle integrates
the unpadded frames: the maps must be equal bit for bit (compare_maps(exact=True)).  The host entry points are driven through
ctypes with buffers that END WITH THE LAST PIXEL of the last row (the header's rule: an image is (height - 1) * row_stride + width
pixels long); tests/test_host_math.py checks the span arithmetic itself under the sanitizers."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import SDEF
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

ERR_INVALID = -1  # (mlmap_hip.h)
# two image widths: 333 is no multiple of 32 (the last tile of a row is cut, mlm_tile_of), 640 is
CFGS = {333: SDEF.with_(width=333, height=200, cam_cx=166.5, cam_cy=100.0, depth_noise_coe=0.00375, lm_occupied_sh=2.0),
        640: SDEF.with_(depth_noise_coe=0.00375, lm_occupied_sh=2.0)}
MODES = {"sectors": {}, "cell-tables": {"sectors": 0}, "no-graph": {"graph": 0}, "cell-tables-no-graph": {"sectors": 0, "graph": 0}}


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


class Scene:
    """frames of the jittered room along a smooth trajectory, and padded copies of them"""

    def __init__(self, cfg, seed):
        self.cfg, self.seed, self.k = cfg, seed, 0
        self.base = syn.room_depth(cfg)
        self.traj = syn.smooth_trajectory(64, seed)
        self.rng = np.random.default_rng(seed)

    def frames(self, n):
        fr = [syn.jitter_depth(self.base, self.k + j, seed=self.seed) for j in range(n)]
        q = np.stack([self.traj[self.k + j][0] for j in range(n)])
        t = np.stack([self.traj[self.k + j][1] + [0.03 * (self.k + j), 0.0, 0.0] for j in range(n)])
        self.k += n
        return np.stack(fr), q, t

    def pad(self, frames, row_stride, gap=0, trim=True):
        """the frames in one flat buffer, rows row_stride apart and frames row_stride * H + gap apart, everything between the
        pixels random valid depth; trim: the buffer ends with the last pixel of the last frame.  -> (buffer, frame_stride)"""
        n, H, W = frames.shape
        fs = row_stride * H + gap
        buf = self.rng.integers(300, 6000, size=n * fs).astype(np.uint16)
        for k in range(n):
            rows = buf[k * fs:k * fs + row_stride * H].reshape(H, row_stride)
            rows[:, :W] = frames[k]
        assert (buf != 0).all() or (frames == 0).any()
        if trim:
            buf = buf[:(n - 1) * fs + (H - 1) * row_stride + W].copy()
        return buf, fs


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _to_device(buf):
    import torch

    d = torch.from_numpy(buf.view(np.int16)).cuda()
    torch.cuda.synchronize()
    return d


def drive_every_entry_point(MLMap, OracleMap, cfg, seed, what):
    """every entry point with padded images on one handle, the map compared with the oracle's after each"""
    W, H = cfg.width, cfg.height
    gpu, cpu = MLMap(cfg, max_blocks=2048, max_points=W * H, max_batch=4), OracleMap(cfg)
    L, h = gpu._L, gpu._h
    sc = Scene(cfg, seed)

    def oracle(fr, q, t, pix=None):
        for k in range(len(fr)):
            if pix is None:
                cpu.update_depth(fr[k], q[k], t[k])
            else:
                cpu.update_depth_indexed(fr[k], pix, q[k], t[k])

    def same(stage):
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"{what}: {stage}", exact=True)
        if cfg.use_exploration_frontiers:
            assert np.array_equal(gpu.export_frontier(), cpu.export_frontier()), f"{what}: {stage}: frontier sets differ"

    # mlm_integrate_depth_u16_dev
    for rs in (W + 1, W + 7, 2 * W):
        fr, q, t = sc.frames(1)
        buf, _ = sc.pad(fr, rs)
        d = _to_device(buf)
        gpu.update_map_dev(d.data_ptr(), W, H, q[0], t[0], row_stride=rs)
        gpu.sync()
        del d
        oracle(fr, q, t)
        same(f"update_map_dev row_stride={rs}")
    # mlm_integrate_depth_batch_dev: padded rows and a gap between the frames; then padded rows and the default frame_stride
    # (row_stride * H: the wrapper's default must follow the row stride)
    for rs, gap in ((W + 5, 3 * W + 11), (W + 3, 0)):
        fr, q, t = sc.frames(5)
        buf, fs = sc.pad(fr, rs, gap)
        d = _to_device(buf)
        if gap:
            gpu.update_map_batch_dev(d.data_ptr(), 5, W, H, q, t, frame_stride=fs, row_stride=rs)
        else:
            gpu.update_map_batch_dev(d.data_ptr(), 5, W, H, q, t, row_stride=rs)
        gpu.sync()
        del d
        oracle(fr, q, t)
        same(f"update_map_batch_dev row_stride={rs} gap={gap}")
    # mlm_integrate_depth_u16, dense and with a pixel list (indices v * width + u, whatever the stride)
    for rs, sampled in ((W + 7, False), (W + 1, True), (2 * W, True)):
        fr, q, t = sc.frames(1)
        buf, _ = sc.pad(fr, rs)
        pix = (sc.rng.integers(0, H, 700) * W + sc.rng.integers(0, W, 700)).astype(np.int32) if sampled else None
        rc = L.mlm_integrate_depth_u16(h, _ptr(buf), W, H, rs, None if pix is None else _ptr(pix), 0 if pix is None else pix.size,
                                       _ptr(_f64(q[0])), _ptr(_f64(t[0])))
        assert rc == 0, (what, rs, sampled, rc)
        oracle(fr, q, t, pix)
        same(f"mlm_integrate_depth_u16 row_stride={rs} sampled={sampled}")
    # mlm_integrate_depth_batch: packed (frame_stride == row_stride * H: one upload per chunk) with the last row of the last frame
    # not padded, six frames in chunks of four and two; gapped; packed with the last row padded
    for rs, gap, trim, n in ((W + 7, 0, True, 6), (W + 1, 2 * W + 9, True, 5), (W + 2, 0, False, 3)):
        fr, q, t = sc.frames(n)
        buf, fs = sc.pad(fr, rs, gap, trim)
        rc = L.mlm_integrate_depth_batch(h, _ptr(buf), n, fs, W, H, rs, _ptr(_f64(q)), _ptr(_f64(t)))
        assert rc == 0, (what, rs, gap, trim, rc)
        oracle(fr, q, t)
        same(f"mlm_integrate_depth_batch row_stride={rs} gap={gap} trimmed={trim}")
    st = gpu.frame_stats()
    gpu.close()
    return st


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("width", list(CFGS))
def test_padded_images_every_entry_point(mods, knobs, width, mode):
    """both Stage A paths (knob sectors), with the single-frame graph and without (knob graph), at both widths"""
    MLMap, OracleMap = mods
    for k, v in MODES[mode].items():
        knobs.set(k, v)
    st = drive_every_entry_point(MLMap, OracleMap, CFGS[width], 7 + width, f"width {width}, {mode}")
    assert st["n_sector_fallbacks"] == 0, st
    if "graph" in MODES[mode]:
        assert st["n_graph_launches"] == 0, st
    elif mode == "sectors":  # (the default handle: single frames went through the captured graph)
        assert st["n_graph_launches"] > 0, st


def test_padded_images_frontier_mode(mods):
    MLMap, OracleMap = mods
    drive_every_entry_point(MLMap, OracleMap, CFGS[333].with_(use_exploration_frontiers=True), 5, "width 333, frontier mode")


def test_padded_images_async_mode(mods):
    """asynchronous mode: the caller's padded host buffers are read by the uploads only, and may change once a call returns"""
    MLMap, OracleMap = mods
    cfg = CFGS[333]
    W, H = cfg.width, cfg.height
    gpu, cpu = MLMap(cfg, max_blocks=2048, max_points=W * H, max_batch=4), OracleMap(cfg)
    gpu.set_async(True)
    sc = Scene(cfg, 11)
    for rs, gap, n in ((W + 7, 0, 6), (W + 1, W + 3, 5)):
        fr, q, t = sc.frames(n)
        buf, fs = sc.pad(fr, rs, gap)
        rc = gpu._L.mlm_integrate_depth_batch(gpu._h, _ptr(buf), n, fs, W, H, rs, _ptr(_f64(q)), _ptr(_f64(t)))
        assert rc == 0
        buf[:] = 777  # (the call has returned: the buffer is the caller's again)
        for k in range(n):
            cpu.update_depth(fr[k], q[k], t[k])
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "async, padded host batches", exact=True)
    gpu.close()


def test_batch_dev_default_frame_stride_follows_row_stride(mods):
    """regression: update_map_batch_dev(row_stride=rs) without frame_stride used width * height between the frames, so that padded
    frames overlapped — every frame after the first was read from the wrong place"""
    MLMap, OracleMap = mods
    cfg = CFGS[333]
    W, H = cfg.width, cfg.height
    gpu, cpu = MLMap(cfg, max_blocks=2048, max_points=W * H, max_batch=4), OracleMap(cfg)
    sc = Scene(cfg, 3)
    fr, q, t = sc.frames(3)
    buf, fs = sc.pad(fr, W + 9, trim=False)
    assert fs == (W + 9) * H
    d = _to_device(buf)
    gpu.update_map_batch_dev(d.data_ptr(), 3, W, H, q, t, row_stride=W + 9)
    gpu.sync()
    for k in range(3):
        cpu.update_depth(fr[k], q[k], t[k])
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "default frame_stride", exact=True)
    gpu.close()


def test_row_stride_below_width_is_refused(mods):
    """row_stride < width: MLM_ERR_INVALID on all four depth entry points, and the handle keeps working"""
    MLMap, OracleMap = mods
    cfg = CFGS[333]
    W, H = cfg.width, cfg.height
    gpu, cpu = MLMap(cfg, max_blocks=2048, max_points=W * H, max_batch=4), OracleMap(cfg)
    L, h = gpu._L, gpu._h
    sc = Scene(cfg, 2)
    fr, q, t = sc.frames(2)
    host = np.ascontiguousarray(fr)
    d = _to_device(host.reshape(-1))
    pq, pt = _ptr(_f64(q)), _ptr(_f64(t))
    dp = ctypes.c_void_p(d.data_ptr())
    for rs in (W - 1, 1, 0, -W):
        assert L.mlm_integrate_depth_u16(h, _ptr(host), W, H, rs, None, 0, pq, pt) == ERR_INVALID, rs
        assert L.mlm_integrate_depth_u16_dev(h, dp, W, H, rs, None, 0, pq, pt) == ERR_INVALID, rs
        assert L.mlm_integrate_depth_batch(h, _ptr(host), 2, W * H, W, H, rs, pq, pt) == ERR_INVALID, rs
        assert L.mlm_integrate_depth_batch_dev(h, dp, 2, W * H, W, H, rs, pq, pt) == ERR_INVALID, rs
    assert gpu.block_count() == 0
    gpu.update_map_batch(fr, q, t)
    for k in range(2):
        cpu.update_depth(fr[k], q[k], t[k])
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "after the refused calls", exact=True)
    gpu.close()
