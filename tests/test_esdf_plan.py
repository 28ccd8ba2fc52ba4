"""mlm_export_esdf's tile planner and its interface, on the CPU.

* mlm_esdf_plan (mlmapping_amd/csrc/mlm_host.h) built with g++ -fsanitize=address,undefined over a sweep of window dims, C,
  gradients on / off, voxel caps (the default, the smallest the esdf_tile_vox knob admits, one in between) and the staging cap:
  every window voxel lies in exactly one tile, every tile's output is one contiguous range of the window's layout, no grown tile
  exceeds the voxel cap and no staged tile the staging cap.
* the knob's range, the binding's methods and flag constants.
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


BOX, MIN_BOX, STAGE = _host_const("kEsdfBoxVoxels"), _host_const("kEsdfMinBoxVoxels"), _host_const("kEsdfStageVoxels")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ep") / "esdf_plan_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "esdf_plan_driver.cpp"), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
        return np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)

    return run


def tiles(D, T):
    """(origin, dims) of every tile, in the host's order"""
    for z0 in range(0, D[2], T[2]):
        for y0 in range(0, D[1], T[1]):
            for x0 in range(0, D[0], T[0]):
                o = (x0, y0, z0)
                yield o, tuple(min(T[a], D[a] - o[a]) for a in range(3))


def check_rows(rows):
    D, C, grad, box, out = rows[:, 0:3], rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6]
    T, n, H, grown = rows[:, 7:10], rows[:, 10:13], rows[:, 13], rows[:, 14]
    assert (T >= 1).all() and (T <= D).all()
    assert (n == -(-D // T)).all()
    assert (H == C - 1 + grad).all()
    assert (grown == np.prod(T + 2 * H[:, None], axis=1)).all()
    assert (grown <= box).all(), "a grown tile exceeds the voxel cap"
    staged = out > 0
    assert (np.prod(T, axis=1)[staged] <= out[staged]).all(), "a staged tile exceeds the staging cap"
    # contiguous outputs: pieces of one row, rows of one plane, or whole planes
    assert ((T[:, 0] == D[:, 0]) | ((T[:, 1] == 1) & (T[:, 2] == 1))).all()
    assert ((T[:, 1] == D[:, 1]) | (T[:, 2] == 1)).all()
    # whole planes whenever one grown plane fits (no needless tiles)
    plane_fits = ((D[:, 0] + 2 * H) * (D[:, 1] + 2 * H) * (1 + 2 * H) <= box) & (~staged | (D[:, 0] * D[:, 1] <= out))
    assert ((T[:, 0] == D[:, 0]) & (T[:, 1] == D[:, 1]))[plane_fits].all()


def test_plan_sweep(driver):
    rows = driver("sweep")
    assert len(rows) > 10000
    assert set(rows[:, 5]) >= {BOX, MIN_BOX}
    check_rows(rows)
    # several tiles happen, with every kind of cut
    T, D = rows[:, 7:10], rows[:, 0:3]
    assert (T[:, 0] < D[:, 0]).any() and (T[:, 1] < D[:, 1]).any() and (T[:, 2] < D[:, 2]).any()


@pytest.mark.parametrize("C,grad,box,out", [(1, 0, MIN_BOX, 0), (5, 1, MIN_BOX, 0), (16, 1, MIN_BOX, 0), (32, 1, MIN_BOX, 0),
                                            (64, 1, MIN_BOX, 0), (64, 0, MIN_BOX, STAGE), (16, 0, BOX, 50), (3, 1, 2 * MIN_BOX, 7)])
def test_plan_covers_each_voxel_once(driver, C, grad, box, out):
    """small windows at small caps: the tiles, enumerated as the host does, cover every voxel once, each with one contiguous
    range of the window's flat layout"""
    cases = [(1, 1, 1), (3, 1, 1), (1, 1, 9), (40, 3, 2), (61, 37, 5), (130, 17, 3), (300, 1, 4), (9, 200, 2)]
    args = [v for d in cases for v in (*d, C, grad, box, out)]
    rows = driver(*args)
    check_rows(rows)
    for r in rows:
        D, T = tuple(int(v) for v in r[0:3]), tuple(int(v) for v in r[7:10])
        cover = np.zeros((D[2], D[1], D[0]), dtype=np.int32)
        count = 0
        for o, td in tiles(D, T):
            sl = cover[o[2]:o[2] + td[2], o[1]:o[1] + td[1], o[0]:o[0] + td[0]]
            sl += 1
            zz, yy, xx = np.unravel_index(np.arange(td[0] * td[1] * td[2]), (td[2], td[1], td[0]))
            idx = ((o[2] + zz) * D[1] + o[1] + yy) * D[0] + o[0] + xx
            base = (o[2] * D[1] + o[1]) * D[0] + o[0]
            assert np.array_equal(idx, base + np.arange(idx.size)), (D, T, o)  # one contiguous range from the tile's first voxel
            count += 1
        assert (cover == 1).all(), (D, T)
        assert count == int(np.prod(r[10:13]))


def test_knob_range():
    """esdf_tile_vox: any cap from the smallest the planner honours for every call up to the default; outside it refused"""
    from mlmapping_amd.mlmap import load_library

    L = load_library()
    try:
        for v in (MIN_BOX, MIN_BOX + 1, 1 << 24, BOX):
            assert L.mlm_debug_set(b"esdf_tile_vox", v) == 0, v
        for v in (-1, 0, 1, 27, MIN_BOX - 1, BOX + 1, 1 << 40):
            assert L.mlm_debug_set(b"esdf_tile_vox", v) == -1, v
    finally:
        L.mlm_debug_reset()
    assert MIN_BOX == (2 * 64 + 1) ** 3  # one voxel grown by the largest H (C = 64 with gradients)


def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_ESDF_OCC, mlmap.MLM_ESDF_INFL, mlmap.MLM_ESDF_UNKNOWN, mlmap.MLM_ESDF_SIGNED) == (1, 2, 4, 8)
    assert callable(mlmap.MLMap.export_esdf) and callable(mlmap.MLMap.export_esdf_dev)
    assert "mlm_export_esdf" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_esdf")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("OCC", 1), ("INFL", 2), ("UNKNOWN", 4), ("SIGNED", 8)):
        assert re.search(rf"#define MLM_ESDF_{name} {v}\b", hdr), name
