"""k_bin_sectors' wave merge: the lanes of a wave (an 8x8 pixel tile of a dense image) that share a centre cell become ONE record, held
by the group's lowest lane and carrying the group's 64-bit lane mask; points beyond the map that still cast a ray are merged the same
way per identical start.  Dense frames of 8x8 (one wave), 32x8 (one full strip), 9x9 and 40x16 pixels (partial waves, several
strips) on the S1 map, with the group shapes the peel loops can meet: one group of 64 lanes, 64 groups of one, holes (depth 0) at
lane 0, at lane 63 and in a checkerboard, and frames that only have ray starts outside the map.  Hit sets, hit odds (float bits),
miss sets and the map's log-odds (float bits) against the oracle.  Reference: src/map_awareness.cpp:173-282."""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (32, 8), (9, 9), (40, 16)]  # (width, height)
# yaw 10.5 degrees, level: the optical axis points at the middle of azimuth cell 10 and of the z cell around the sensor's height
POSE = syn.quat_from_rpy(0.0, 0.0, np.radians(10.5)), np.array([0.0, 0.0, 1.5])


def _cfg(w, h, f):
    return S1.with_(width=w, height=h, cam_cx=w / 2 - 0.5, cam_cy=h / 2 - 0.5, cam_fx=f, cam_fy=f)


def _wall(w, h, raw=1030):
    """a wall at 1.03 m seen with a focal length of 4 000 pixels: the whole image spans 0.6 degrees and 5 mm — every pixel of a wave
    (of the image) falls into the one cell around rho = 1.15 m"""
    return np.full((h, w), raw, dtype=np.uint16)


def _scenes(w, h):
    rng = np.random.default_rng(w * 100 + h)
    out = {"wall": (_cfg(w, h, 4000.0), _wall(w, h))}
    sc = syn.ScatterScene(_cfg(w, h, 385.0))
    out["scatter"] = (_cfg(w, h, 385.0), sc.next())
    # every lane its own cell for certain: a focal length of 40 pixels puts neighbouring columns 1.4 degrees apart (azimuth cells of one
    # degree), and the rows of an 8x8 tile lie 0.6 m apart in depth (range steps of 0.1 m)
    yy = np.mgrid[0:h, 0:w][0]
    out["scatter_wide"] = (_cfg(w, h, 40.0), (1000 + (yy % 8) * 600 + rng.integers(0, 90, (h, w))).astype(np.uint16))
    for name in ("hole_lane0", "hole_lane63", "checkerboard"):
        for base, (cfg, img) in (("wall", out["wall"]), ("scatter", out["scatter"])):
            img = img.copy()
            if name == "hole_lane0":
                img[0::8, 0::8] = 0  # (lane 0 of every 8x8 tile)
            elif name == "hole_lane63":
                img[7::8, 7::8] = 0
                img[h - 1, w - 1] = 0  # (and the last pixel of a partial tile)
            else:
                yy, xx = np.mgrid[0:h, 0:w]
                img[(yy + xx) % 2 == 0] = 0
            out[f"{base}_{name}"] = (cfg, img)
    # beyond the map (nRho * dRho = 6.5 m) but casting: one start per wave (far wall), and starts that differ from lane to lane
    out["outer_wall"] = (_cfg(w, h, 4000.0), _wall(w, h, 9000))
    out["outer_scatter"] = (_cfg(w, h, 40.0), (8000 + rng.permutation(w * h).reshape(h, w) * 20).astype(np.uint16))
    return out


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_wave_merge_group_shapes(w, h):
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    maps = {}  # one map per camera: its scenes follow each other (a later frame meets the earlier ones' voxels)
    for name, (cfg, img) in _scenes(w, h).items():
        if cfg.cam_fx not in maps:
            maps[cfg.cam_fx] = MLMap(cfg, max_blocks=4096, max_points=4096, record_awareness=True, max_batch=2), OracleMap(cfg)
        gpu, cpu = maps[cfg.cam_fx]
        gpu.update_map(img, *POSE)
        cpu.update_depth(img, *POSE)
        what = f"{w}x{h} {name}"
        gc, go, _ = gpu.awareness_hits()
        cc, co = cpu.hit_cells_sorted()
        assert np.array_equal(gc, cc), f"{what}: hit cells differ"
        assert np.array_equal(go.view(np.uint32), co.view(np.uint32)), f"{what}: hit odds differ in bits"
        assert np.array_equal(gpu.awareness_misses(), np.sort(cpu.misses()).astype(np.int64)), f"{what}: miss cells differ"
        if name == "wall":
            assert 1 <= len(cc) <= 3, (what, len(cc))  # (one centre cell, its spread neighbours if any)
        if name == "scatter_wide":
            assert len(cc) >= w * h, (what, len(cc))  # (a centre cell per pixel, and their spread)
        if name.startswith("outer"):
            assert len(cc) == 0 and len(cpu.misses()) > 0, (what, len(cc), len(cpu.misses()))
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), what)
    for gpu, _ in maps.values():
        assert gpu.frame_stats()["n_sector_fallbacks"] == 0
        gpu.close()
