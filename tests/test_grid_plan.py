"""mlm_export_grid2d's tile planner and its interface, on the CPU.

* mlm_grid_plan (mlmapping_amd/csrc/mlm_host.h) built with g++ -fsanitize=address,undefined over a sweep of plane dims, C,
  distances on / off, box caps (the default, the smallest, one in between) and cell caps (none, the staging cap, small values of the
  grid_tile knob): every cell lies in exactly one tile, every tile's output is one contiguous range of the plane's layout, no grown
  tile exceeds the box cap and no tile the cell cap.
* the knob's range, grid2d_band's triples, the binding's methods and constants.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")


def _host_const(name):
    txt = open(os.path.join(CSRC, "mlm_host.h")).read()
    return eval(re.search(rf"constexpr long long {name} = ([^;]+);", txt).group(1).replace("ll", ""))


BOX, MIN_BOX, STAGE = _host_const("kGridBoxCells"), _host_const("kGridMinBoxCells"), _host_const("kGridStageCells")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gp") / "grid_plan_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "grid_plan_driver.cpp"), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
        return np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)

    return run


def tiles(D, T):
    """(origin, dims) of every tile, in the host's order"""
    for y0 in range(0, D[1], T[1]):
        for x0 in range(0, D[0], T[0]):
            o = (x0, y0)
            yield o, tuple(min(T[a], D[a] - o[a]) for a in range(2))


def check_rows(rows):
    D, C, dist, box, out = rows[:, 0:2], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
    T, n, H, grown = rows[:, 6:8], rows[:, 8:10], rows[:, 10], rows[:, 11]
    assert (T >= 1).all() and (T <= D).all()
    assert (n == -(-D // T)).all()
    assert (H == np.where(dist != 0, C - 1, 0)).all()
    assert (grown == np.prod(T + 2 * H[:, None], axis=1)).all()
    assert (grown <= box).all(), "a grown tile exceeds the box cap"
    capped = out > 0
    assert (np.prod(T, axis=1)[capped] <= out[capped]).all(), "a tile exceeds the cell cap"
    # contiguous outputs: whole rows, or pieces of one row
    assert ((T[:, 0] == D[:, 0]) | (T[:, 1] == 1)).all()
    # the whole plane whenever it fits (no needless tiles)
    fits = ((D[:, 0] + 2 * H) * (D[:, 1] + 2 * H) <= box) & (~capped | (D[:, 0] * D[:, 1] <= out))
    assert (T == D).all(axis=1)[fits].all()


def test_plan_sweep(driver):
    rows = driver("sweep")
    assert len(rows) > 10000
    assert set(rows[:, 4]) >= {BOX, MIN_BOX} and set(rows[:, 5]) >= {0, 1, STAGE}
    check_rows(rows)
    T, D = rows[:, 6:8], rows[:, 0:2]
    assert (T[:, 0] < D[:, 0]).any() and ((T[:, 1] < D[:, 1]) & (T[:, 1] > 1)).any()  # every kind of cut happens


@pytest.mark.parametrize("C,dist,box,out", [(1, 1, MIN_BOX, 0), (5, 1, MIN_BOX, 0), (5, 1, BOX, 1), (64, 1, MIN_BOX, 0), (64, 1, BOX, STAGE),
                                            (16, 0, BOX, 50), (16, 1, BOX, 50), (3, 1, 2 * MIN_BOX, 7), (5, 0, 100, 0)])
def test_plan_covers_each_cell_once(driver, C, dist, box, out):
    """small planes at small caps: the tiles, enumerated as the host does, cover every cell once, each with one contiguous range of
    the plane's flat layout that starts at the tile's first cell"""
    cases = [(1, 1), (3, 1), (1, 9), (40, 3), (70, 45), (61, 37), (130, 17), (300, 1), (9, 200)]
    rows = driver(*[v for d in cases for v in (*d, C, dist, box, out)])
    check_rows(rows)
    for r in rows:
        D, T = tuple(int(v) for v in r[0:2]), tuple(int(v) for v in r[6:8])
        cover = np.zeros((D[1], D[0]), dtype=np.int32)
        count = 0
        for o, td in tiles(D, T):
            cover[o[1]:o[1] + td[1], o[0]:o[0] + td[0]] += 1
            yy, xx = np.unravel_index(np.arange(td[0] * td[1]), (td[1], td[0]))
            assert np.array_equal((o[1] + yy) * D[0] + o[0] + xx, o[1] * D[0] + o[0] + np.arange(td[0] * td[1])), (D, T, o)
            count += 1
        assert (cover == 1).all(), (D, T)
        assert count == int(np.prod(r[8:10]))


def test_no_tile_fits(driver):
    """a box cap below one grown cell, or no cell at all: T[0] == 0, which the entry point refuses"""
    rows = driver(10, 10, 64, 1, MIN_BOX - 1, 0, 10, 10, 5, 1, 80, 0)
    assert (rows[:, 6] == 0).all()


def test_knob_range(driver):
    """grid_tile: any cell cap from one cell up to the staging cap; outside it refused — by the planner's own check and by
    mlm_debug_set"""
    good, bad = (1, 2, 50, 4096, STAGE), (-1, 0, STAGE + 1, 1 << 40)
    rows = driver("knob", *good, *bad)
    assert rows[:, 1].tolist() == [1] * len(good) + [0] * len(bad)
    from mlmapping_amd.mlmap import load_library

    L = load_library()
    try:
        for v in good:
            assert L.mlm_debug_set(b"grid_tile", v) == 0, v
        for v in bad:
            assert L.mlm_debug_set(b"grid_tile", v) == -1, v
    finally:
        L.mlm_debug_reset()
    assert MIN_BOX == (2 * 63 + 1) ** 2 and MIN_BOX <= BOX  # one cell grown by the largest H (C = 64) always fits


def test_band_helper():
    """grid2d_band: layers floor(zmin / d) .. floor(zmax / d), z_ref the middle layer or the vehicle's layer clamped into the band"""
    from mlmapping_amd.mlmap import MLMap, MlmError

    band = MLMap.grid2d_band
    assert band(0.0, 1.0, 0.25) == (0, 5, 2)
    assert band(-0.875, -0.125, 0.25) == (-4, 4, -2)  # negative heights: floor, not truncation
    assert band(-0.35, -0.05, 0.1) == (-4, 4, -2)
    assert band(0.26, 0.49, 0.25) == (1, 1, 1)  # a band inside one layer
    assert band(-0.5, 0.5, 0.25, z_vehicle=-0.3) == (-4, 5, -2)  # use_relative_height: -0.8 .. 0.2, across zero
    assert band(-0.5, 0.5, 0.25, z_vehicle=0.3) == (-1, 5, 1)  # -0.2 .. 0.8
    assert band(0.5, 1.0, 0.25, z_vehicle=1.0) == (6, 3, 6)  # the vehicle below its band: clamped to the lowest layer
    assert band(-1.0, -0.5, 0.25, z_vehicle=1.0) == (0, 3, 2)  # ... above it: the highest
    for lo_z, dims_z, z_ref in (band(-3.0, 7.0, 0.2), band(0.1, 0.1, 0.05, z_vehicle=-2.0)):
        assert dims_z >= 1 and lo_z <= z_ref < lo_z + dims_z
    with pytest.raises(MlmError):
        band(1.0, 0.0, 0.1)
    with pytest.raises(MlmError):
        band(0.0, 1.0, 0.0)


def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_GRID_OCC, mlmap.MLM_GRID_INFL, mlmap.MLM_GRID_UNKNOWN, mlmap.MLM_GRID_DIST_UNOBSERVED, mlmap.MLM_GRID_COL) == (1, 2, 4, 16, 8)
    assert callable(mlmap.MLMap.export_grid2d) and callable(mlmap.MLMap.export_grid2d_dev) and callable(mlmap.MLMap.grid2d_band)
    assert "mlm_export_grid2d" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_grid2d")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("OCC", 1), ("INFL", 2), ("UNKNOWN", 4), ("DIST_UNOBSERVED", 16), ("COL", 8)):
        assert re.search(rf"#define MLM_GRID_{name} {v}\b", hdr), name
    assert "export_grid2d" in open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
