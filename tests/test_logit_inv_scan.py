"""Every float log-odds L of the maps' range [-2, 4.2] (about 2.2e9 of them) through getOdd's narrowing (float)(p / (1 + p)),
p = pow(10, L) (include/mlmap.h:40), on the host: the few thousand L whose quotient lies within 1024 double ulps of a float rounding
midpoint are the only inputs where the device's pow, if it is within 256 ulps of glibc's, can give another float
(tests/cpp/logit_inv_scan.cpp).  tests/test_gpu_query_exact.py feeds every one of them through the kernels."""
import numpy as np

from oracle.binding import OracleMap
from mlmapping_amd.config import S1
from tests.util import float_range, logit_inv_scan


def test_scan_lists_the_hard_cases(tmp_path_factory):
    s = logit_inv_scan(tmp_path_factory.mktemp("scan"))
    L = s["L"]
    assert s["scanned"] == _count(-2.0, 4.2)
    assert 1000 <= L.size <= 20000, L.size
    assert (np.diff(L) > 0).all() and L.min() >= np.float32(-2.0) and L.max() <= np.float32(4.2)
    assert (np.abs(s["m"]) <= 1024).all()
    # the listed odds are the oracle's getOdd (the same glibc pow) bit for bit
    cfg = S1
    C = cfg.cells_per_block
    nb = -(-L.size // C)
    lo = np.zeros(nb * C, dtype=np.float32)
    lo[:L.size] = L
    cpu = OracleMap(cfg)
    keys = np.stack([np.arange(nb), np.zeros(nb), np.zeros(nb)], axis=1).astype(np.int32)
    cpu.import_blocks(keys, lo.reshape(nb, C))
    idx = np.arange(L.size)
    got = cpu.getOddAt(keys[idx // C], (idx % C).astype(np.int32))
    assert np.array_equal(got.view(np.uint32), s["f"].view(np.uint32))
    # where glibc's pow is not correctly rounded (its bound is 0.52 ulp): a correctly rounded device pow would differ from the host
    # there — 3 of the 1 912 hard cases with glibc 2.35, where the true power lies 0.5005 .. 0.5014 ulp from glibc's
    not_cr = L[~s["cr"]]
    assert not_cr.size <= 8, not_cr
    print(f"{L.size} hard cases among {s['scanned']} floats ({s['threads']} threads); glibc's pow not correctly rounded at {not_cr}")


def _count(lo: float, hi: float) -> int:
    """number of float32 values in [lo, hi] (lo < 0 <= hi): -0.0 and +0.0 both counted"""
    return int(np.float32(lo).view(np.uint32)) - 0x80000000 + 1 + int(np.float32(hi).view(np.uint32)) + 1


def test_float_range():
    a = float_range(-1e-44, 1e-44)
    assert np.array_equal(a.view(np.uint32), np.array([0x80000007, 0x80000006, 0x80000005, 0x80000004, 0x80000003, 0x80000002, 0x80000001,
                                                       0x80000000, 0, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint32))
    assert (np.diff(float_range(-2.0, 4.2, 4099)) > 0).all()
    assert float_range(1.0, 2.0).size == (1 << 23) + 1
    assert float_range(-2.0, -1.0).size == (1 << 23) + 1
