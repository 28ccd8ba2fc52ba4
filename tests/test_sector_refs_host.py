"""The integer forms of k_sector's reference pass (mlmapping_amd/csrc/mlm_sector_refs.h) on the CPU, held to the straightforward
forms by tests/cpp/sector_refs_driver.cpp, built with -fsanitize=address,undefined:
  * a cell's packed origin (row and tile column of its first pixel, worked out once per cell instead of once per (record, cell) pair):
    every pixel below 2^21 at widths 1, 7, 8, 640 and 1280; at 8184 and MLM_SEC_MAX_WIDTH both sides of every row end; the last pixels
    below 2^21 at every width; the 64-item rows of the pixel-list mode;
  * the flags of a lane mask's non-empty rows and the rows taken from them by find-first-bit: all 256 row patterns x 1 000 masks;
  * the reference word repacked from a group's shared base: equal to mlm_ref_pack's;
  * the miss passes' w / RW by multiplication."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")


def max_width():
    src = open(os.path.join(CSRC, "mlm_kernels_sector.h")).read()
    xt_bits = int(re.search(r"#define MLM_REC_XT_BITS (\d+)", src).group(1))
    assert "#define MLM_SEC_MAX_WIDTH ((int)(MLM_REC_XT_MASK << 3))" in src
    return ((1 << xt_bits) - 1) << 3


WIDTHS = [1, 7, 8, 640, 1280, 8184]


def test_header_and_kernel_agree_on_the_time_slots():
    """mlm_sector_refs.h restates MLM_TIME_SLOTS for the CPU build (mlm_types.h holds device types): the two must be one value"""
    a = re.search(r"#define MLM_TIME_SLOTS (\d+)", open(os.path.join(CSRC, "mlm_types.h")).read()).group(1)
    b = re.search(r"#define MLM_TIME_SLOTS (\d+)", open(os.path.join(CSRC, "mlm_sector_refs.h")).read()).group(1)
    assert a == b


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("srefs") / "sector_refs_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "sector_refs_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)] + [str(w) for w in WIDTHS + [max_width()]], check=True, capture_output=True, text=True).stdout.split()
    return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}


def test_origin_packing_is_exact(report):
    full = sum(3 * ((1 << 21) // 2) + 2 * ((1 << 21) // 2) for w in WIDTHS if w <= 1280)  # (three kinds per even pixel, two per odd one)
    assert report["n_origin"] > full + 2 * (1 << 21)  # (+ the list mode's items, + the wide images' row ends)
    assert report["n_row_ends"] >= sum(((1 << 21) - 1) // w for w in WIDTHS + [max_width()])
    assert report["bad_origin"] == 0


def test_row_extraction_and_repacked_words(report):
    assert report["n_rows"] == 256 * 1000 and report["bad_rows"] == 0
    assert report["n_repack"] == 1000 * sum(bin(p).count("1") for p in range(256)) and report["bad_repack"] == 0


def test_miss_word_row_by_multiplication(report):
    assert report["n_miss"] == 64 * 65536 and report["bad_miss"] == 0
