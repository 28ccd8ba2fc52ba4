"""strip_magic (mlmapping_amd/csrc/mlm_host.h): k_bin_sectors takes a dense strip's row in the image as the high word of
(2 * strip) * MlmFrame::tx_m instead of dividing by the strips per row.  The multiplier has to be exact for every strip index below
2^20 and every divisor 1 .. 2^11 (the sector path's widest image, 65 528 pixels, has 2 048 strips per row; its largest frame fewer
than 2^15 strips).  The range is below 2^24, so the driver checks it exhaustively: 2 048 divisors x 2^20 operands."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sm") / "strip_magic_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "strip_magic_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}


def test_strip_magic_exact_over_its_whole_range(report):
    assert report["max_i"] == 1 << 20 and report["max_d"] == 1 << 11
    assert report["checked"] == (1 << 20) * (1 << 11) and report["bad"] == 0


def test_strip_magic_refuses_divisors_out_of_range(report):
    """0: the frame has no multiplier (an image wider than the sector path takes is never binned by k_bin_sectors)"""
    assert report["refused"] == 3


def test_strip_magic_range_is_what_the_sector_path_needs():
    """the stated range covers the sector path's limits as the sources define them"""
    import re

    src = open(os.path.join(ROOT, "mlmapping_amd", "csrc", "mlm_kernels_sector.h")).read()
    xt_bits = int(re.search(r"#define MLM_REC_XT_BITS (\d+)", src).group(1))
    host = open(os.path.join(ROOT, "mlmapping_amd", "csrc", "mlm_host.h")).read()  # (the sector path's limits that the host plans with)
    cnt_bits = int(re.search(r"#define MLM_SEC_CNT_BITS (\d+)", host).group(1))
    max_width = ((1 << xt_bits) - 1) << 3                   # MLM_SEC_MAX_WIDTH
    assert (max_width + 31) // 32 <= 1 << 11                # strips per row of the widest image
    assert (1 << cnt_bits) // 128 + 256 <= 1 << 20          # MlmDev::nb_cap with mlm_limits.max_points < 2^MLM_SEC_CNT_BITS
