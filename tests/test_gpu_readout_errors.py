"""The box check of the nine boxed read-outs: a window with a dim < 1, one whose lo + dims leaves the int32 range and one of more
than 2^31 - 1 voxels are refused with MLM_ERR_INVALID and the entry point's own text, and the handle goes on answering."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd.config import SDEF

pytestmark = pytest.mark.gpu

MLM_OK, MLM_ERR_INVALID = 0, -1
BAD_BOX = ": dims must be >= 1 and lo + dims must fit an int32"
TOO_MANY = ": more than 2^31 - 1 voxels"
# (lo, dims, message)
WINDOWS = [((0, 0, 0), (0, 1, 1), BAD_BOX), (((1 << 31) - 2, 0, 0), (2, 1, 1), BAD_BOX), ((0, 0, 0), (65536, 32768, 1), TOO_MANY)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def gpu():
    from mlmapping_amd.mlmap import MLMap

    m = MLMap(SDEF, max_blocks=2048)  # (no frame integrated: an empty map)
    yield m
    m.close()


def _calls(L, h):
    """name -> call(lo, dims) with otherwise valid arguments and outputs of 8 elements"""
    f32, i8, i32, i64, u8 = (np.zeros(8, dtype=t) for t in (np.float32, np.int8, np.int32, np.int64, np.uint8))
    seeds, goal, box6 = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32), np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    move_cost = np.ones(3, dtype=np.int32)
    p0, p1, view_begin = np.zeros(3), np.ones(3), np.array([0, 1], dtype=np.int32)
    keep = [f32, i8, i32, i64, u8, seeds, goal, box6, move_cost, p0, p1, view_begin]
    return keep, {
        "mlm_export_window": lambda lo, d: L.mlm_export_window(h, lo, d, 0, _p(f32), None, None, None),
        "mlm_export_esdf": lambda lo, d: L.mlm_export_esdf(h, lo, d, 4, 1, _p(i32), None, None),
        "mlm_export_grid2d": lambda lo, d: L.mlm_export_grid2d(h, lo, d, 1, 0, 0, 1, _p(i8), None, None, None, None),
        "mlm_export_reach": lambda lo, d: L.mlm_export_reach(h, lo, d, _p(seeds), 1, 1, 0, 8, _p(i32), None, None),
        "mlm_export_route": lambda lo, d: L.mlm_export_route(h, lo, d, _p(seeds), 1, 1, 0, 6, _p(move_cost), None, 0, 100, _p(i32), None, None),
        "mlm_export_clusters": lambda lo, d: L.mlm_export_clusters(h, lo, d, 1, 6, 1, _p(i32), None, 0, None),
        "mlm_query_boxes": lambda lo, d: L.mlm_query_boxes(h, _p(box6), 1, 1, None, lo, d, _p(i8), None, None, None),
        "mlm_query_paths": lambda lo, d: L.mlm_query_paths(h, lo, d, _p(u8), 0, _p(goal), 1, 1, 8, 0, _p(i8), None, None, None),
        "mlm_query_views": lambda lo, d: L.mlm_query_views(h, _p(p0), _p(p1), _p(view_begin), 1, 1, lo, d, None, None, _p(i64)),
    }


@pytest.mark.parametrize("name", ["mlm_export_window", "mlm_export_esdf", "mlm_export_grid2d", "mlm_export_reach", "mlm_export_route",
                                  "mlm_export_clusters", "mlm_query_boxes", "mlm_query_paths", "mlm_query_views"])
def test_bad_boxes_are_refused(gpu, name):
    L, h = gpu._L, gpu._h
    keep, calls = _calls(L, h)
    for lo, dims, text in WINDOWS:
        lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
        assert calls[name](_p(lo_a), _p(dims_a)) == MLM_ERR_INVALID, (name, lo, dims)
        assert L.mlm_last_error(h).decode() == name + text, (name, lo, dims)
    # the handle still answers
    lo_a, dims_a, odds = np.zeros(3, dtype=np.int32), np.full(3, 2, dtype=np.int32), np.full(8, np.nan, dtype=np.float32)
    assert L.mlm_export_window(h, _p(lo_a), _p(dims_a), 0, _p(odds), None, None, None) == MLM_OK
    assert np.isfinite(odds).all()
    del keep
