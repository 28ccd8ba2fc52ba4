"""The constants that tests/test_gpu_query_ops.py restates from the library's headers, and the host's rule for k_sweeps' slot cache,
read from the sources themselves (no GPU)."""
import os
import re

from tests import test_gpu_query_ops as q
from tests.test_gpu_sweeps import BOUNDARY

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlmapping_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, pattern):
    """the value of the one integer expression that `pattern` captures"""
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    assert re.fullmatch(r"[0-9 ()*+\-]+", found[0]), found[0]
    return eval(found[0])  # (digits, brackets and + - * only)


def test_constants_are_the_headers():
    assert constant(source("mlm_kernels_sweeps.h"), r"constexpr int kSweepNB = ([^;]+);") == q.SWEEP_NB
    assert constant(source("mlm_views.h"), r"constexpr long long kViewLdsBits = ([^;]+);") == q.VIEW_LDS_BITS
    handle = source("mlm_plan.h")  # (MlmMirrorLimits: the limits mlm_handle.h's MlmMirror derives from)
    assert constant(handle, r"int max_clean = ([^;]+);") == 4 * q.MIRROR_CLEAN and constant(handle, r"int max_dirty = ([^;]+);") == 4 * 8
    # a batch of boxes, points, rays or poses takes four of those units per item
    assert source("mlm_mirror.h").count("n * 4 > (M.dirty ? M.max_dirty : M.max_clean)") + \
        source("mlm_mirror.h").count("n_poses * 4 > (M.dirty ? M.max_dirty : M.max_clean)") == 5


def test_cached_radius_is_the_host_rule():
    """cached_radius() is the rule as mlm_query_sweeps states it, and the crafted cases stand on either side of it"""
    assert "cached = radius > 0 && (2 * radius - 1) / h->P.n + 2 <= kSweepNB;" in source("mlmap_hip.hip")
    assert [q.cached_radius(n) for n in (2, 3, 4, 5, 7, 8, 10, 16)] == [4, 6, 8, 10, 14, 16, 16, 16]
    for n in (2, 3, 4, 7):
        assert (n, q.cached_radius(n)) in BOUNDARY and (n, q.cached_radius(n) + 1) in BOUNDARY
