"""A column's four list reservations (k_sector: hits, ranked cells, references, contributions) and a tile's two (k_tile: voxel
records, entries of vr_hit) each leave in ONE returning add whose lanes take one counter each; a lane with nothing to reserve is
masked off.  The cases: three of a column's four amounts zero, all four non-zero, a tile with nothing for vr_hit, and both widths
of k_sector's workgroup — every map equal to the oracle's bit for bit, no frame on the cell-table path."""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1, S1_SIGMA0
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

W, H = 160, 120
CAM = dict(width=W, height=H, cam_cx=W / 2.0, cam_cy=H / 2.0, cam_fx=385.0 / 4, cam_fy=385.0 / 4)  # S1's camera at a quarter of its resolution
CFG_ONE_KIND = S1_SIGMA0.with_(**CAM)  # no depth noise: a hit reaches its own cell only — no cell has two kinds of contribution
CFG_KINDS = S1.with_(**CAM)
# one 32x8-pixel strip, its pixels' rays a voxel and more apart at the walls: a tile's voxels hold one hit each
CFG_STRIP = S1.with_(width=32, height=8, cam_cx=16.0, cam_cy=4.0, cam_fx=20.0, cam_fy=20.0)


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


_REF = {}


def reference(OracleMap, name, cfg, frames):
    """the oracle's map after `frames`, computed once per module"""
    if name not in _REF:
        cpu = OracleMap(cfg)
        for img, (q, t) in frames:
            cpu.update_depth(img, q, t)
        _REF[name] = cpu.export_blocks()
    return _REF[name]


def feed(gpu, frames, batched):
    if batched:
        gpu.set_async(True)
        gpu.update_map_batch(np.stack([f[0] for f in frames]), np.stack([f[1][0] for f in frames]), np.stack([f[1][1] for f in frames]))
    else:
        for img, (q, t) in frames:
            gpu.update_map(img, q, t)


@pytest.mark.parametrize("how", ["one asynchronous batch", "frame by frame"])
def test_three_of_a_columns_four_lanes_masked_off(mods, how):
    """S1_SIGMA0: every hit cell has one kind — n_multi, the references and the contributions are zero in every column, only the lane
    of the hit list reserves"""
    MLMap, OracleMap = mods
    frames = list(syn.stream(CFG_ONE_KIND, "room_jitter", "smooth", 4))
    gpu = MLMap(CFG_ONE_KIND, max_blocks=2048, max_points=W * H, max_batch=4)
    feed(gpu, frames, how == "one asynchronous batch")
    compare_maps(gpu.export_blocks(), reference(OracleMap, "one kind", CFG_ONE_KIND, frames), how, exact=True)
    st = gpu.frame_stats()
    assert st["n_multi_cells"] == 0 and st["n_hit_cells"] > 0, st
    assert st["n_sector_fallbacks"] == 0, st
    gpu.close()


@pytest.mark.parametrize("how", ["max_batch 1: 512 threads", "in a batch: 256 threads"])
def test_all_four_amounts_and_both_workgroup_widths(mods, how):
    """S1: cells with several kinds of contribution — every lane reserves; a lone frame's columns run 512 threads wide, a batch's 256"""
    MLMap, OracleMap = mods
    frames = list(syn.stream(CFG_KINDS, "room_jitter", "smooth", 4))
    batched = how.startswith("in a batch")
    gpu = MLMap(CFG_KINDS, max_blocks=2048, max_points=W * H, max_batch=4 if batched else 1)
    feed(gpu, frames, batched)
    compare_maps(gpu.export_blocks(), reference(OracleMap, "kinds", CFG_KINDS, frames), how, exact=True)
    st = gpu.frame_stats()
    assert st["n_multi_cells"] > 0, st
    assert st["n_sector_fallbacks"] == 0, st
    gpu.close()


def test_one_strip_frame_alone(mods):
    """32x8 pixels: a handful of columns and tiles, the tiles' voxels with one hit each — the lane of vr_hit stays masked off"""
    MLMap, OracleMap = mods
    frames = list(syn.stream(CFG_STRIP, "room_jitter", "smooth", 2))
    gpu = MLMap(CFG_STRIP, max_blocks=2048, max_points=32 * 8, max_batch=1)
    feed(gpu, frames, False)
    compare_maps(gpu.export_blocks(), reference(OracleMap, "strip", CFG_STRIP, frames), "one-strip frames", exact=True)
    st = gpu.frame_stats()
    assert st["n_hit_cells"] > 0 and st["n_sector_fallbacks"] == 0, st
    gpu.close()


def test_one_strip_frame_between_batches(mods):
    """the same strip as a submission of its own between asynchronous batches of 160x120 frames (a batch shares one geometry)"""
    MLMap, OracleMap = mods
    big = list(syn.stream(CFG_KINDS, "room_jitter", "smooth", 4))
    strip = [(img, big[2 + k][1]) for k, (img, _) in enumerate(syn.stream(CFG_STRIP, "room_jitter", "smooth", 2))]
    seq = big[:2] + strip + big[2:]
    gpu = MLMap(CFG_KINDS, max_blocks=2048, max_points=W * H, max_batch=4)
    feed(gpu, big[:2], True)
    feed(gpu, strip, True)
    feed(gpu, big[2:], True)
    compare_maps(gpu.export_blocks(), reference(OracleMap, "strip between batches", CFG_KINDS, seq), "strip between batches", exact=True)
    assert gpu.frame_stats()["n_sector_fallbacks"] == 0
    gpu.close()
