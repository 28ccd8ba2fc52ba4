"""k_bin_sectors takes a dense pixel's column and row from the strip's place in the image (strip row by MlmFrame::tx_m, no division):
small dense images at the widths where that geometry can go wrong, against the oracle bit for bit (compare_maps(exact=True)).

* widths that are no multiple of 32 or of 8 (33 x 9, 40 x 24, 71 x 17: the last strip of a row and the last wave of a strip are cut),
  a width below 32 (24 x 8, which is also a single strip), an exact multiple (64 x 16) and one full strip (32 x 8);
* every shape once frame by frame (the strip index is blockIdx.x of a lone frame's launch, the parameters come from pinned memory) and once
  as an asynchronous batch of four (one launch, blockIdx.z = frame slot);
* padded images (row_stride > width, the padding random valid depths) through the device-buffer entry points, single and batched.

Depths are random per pixel (neighbouring pixels land in different cells and columns) with some zero (invalid) pixels.  Every case asserts
that no frame left the sector path, so it cannot pass on the cell-table kernels."""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

SHAPES = [(33, 9), (40, 24), (71, 17), (24, 8), (64, 16), (32, 8)]  # (width, height)
N_FRAMES = 4


def _cfg(W, H):
    # a 40 degree wide view whatever the size: a frame's few pixels spread over tens of azimuth columns (1 degree each), a 32 x 8 strip
    # stays well below the 64 columns its table takes
    f = 0.5 * W / np.tan(np.radians(20.0))
    return S1.with_(width=W, height=H, cam_cx=W / 2.0, cam_cy=H / 2.0, cam_fx=float(f), cam_fy=float(f))


def _frames(W, H, seed):
    rng = np.random.default_rng(seed)
    fr = rng.integers(500, 6000, size=(N_FRAMES, H, W)).astype(np.uint16)
    fr[rng.random(fr.shape) < 0.05] = 0  # (invalid pixels, mlmap.cpp:338-341)
    traj = syn.smooth_trajectory(N_FRAMES, seed)
    q = np.stack([traj[k][0] for k in range(N_FRAMES)])
    t = np.stack([traj[k][1] + [0.05 * k, 0.0, 0.0] for k in range(N_FRAMES)])
    return fr, q, t


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


@pytest.fixture(scope="module")
def want(mods):
    """{(W, H): (frames, q, t, the oracle's map after them)}, computed once per shape"""
    _, OracleMap = mods
    cache = {}

    def get(W, H):
        if (W, H) not in cache:
            fr, q, t = _frames(W, H, 100 * W + H)
            cpu = OracleMap(_cfg(W, H))
            for k in range(N_FRAMES):
                cpu.update_depth(fr[k], q[k], t[k])
            cache[(W, H)] = (fr, q, t, cpu.export_blocks())
        return cache[(W, H)]

    return get


def _check(gpu, ref, what):
    gpu.sync()
    st = gpu.frame_stats()
    assert st["n_sector_fallbacks"] == 0, (what, st)
    g = gpu.export_blocks()
    assert len(g["keys"]) > 0, what
    compare_maps(g, ref, what, exact=True)


def _padded(fr, rs, seed):
    """the frames in one flat buffer, rows rs apart, the padding random valid depths"""
    n, H, W = fr.shape
    buf = np.random.default_rng(seed).integers(300, 6000, size=n * rs * H).astype(np.uint16)
    buf.reshape(n, H, rs)[:, :, :W] = fr
    return buf


def _to_device(buf):
    import torch

    d = torch.from_numpy(buf.view(np.int16)).cuda()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("how", ["frame_by_frame", "async_batch"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_strip_geometry(mods, want, shape, how):
    MLMap, _ = mods
    W, H = shape
    fr, q, t, ref = want(W, H)
    gpu = MLMap(_cfg(W, H), max_blocks=2048, max_points=W * H, max_batch=N_FRAMES)
    try:
        if how == "frame_by_frame":
            for k in range(N_FRAMES):
                gpu.update_map(fr[k], q[k], t[k])
        else:
            gpu.set_async(True)
            gpu.update_map_batch(fr, q, t)
        _check(gpu, ref, f"{W}x{H} {how}")
    finally:
        gpu.close()


@pytest.mark.parametrize("how", ["frame_by_frame", "batch"])
def test_dense_strip_geometry_padded_device_image(mods, want, how):
    """row_stride > width through mlm_integrate_depth_u16_dev / mlm_integrate_depth_batch_dev: the image address is row * row_stride +
    column, the work item row * width + column"""
    MLMap, _ = mods
    W, H = 71, 17
    fr, q, t, ref = want(W, H)
    rs = W + 5
    d = _to_device(_padded(fr, rs, 9))
    gpu = MLMap(_cfg(W, H), max_blocks=2048, max_points=W * H, max_batch=N_FRAMES)
    try:
        if how == "frame_by_frame":
            for k in range(N_FRAMES):
                gpu.update_map_dev(d.data_ptr() + 2 * k * rs * H, W, H, q[k], t[k], row_stride=rs)
        else:
            gpu.update_map_batch_dev(d.data_ptr(), N_FRAMES, W, H, q, t, row_stride=rs)
        _check(gpu, ref, f"{W}x{H} padded to {rs}, {how}")
    finally:
        gpu.close()
        del d
