"""k_sector's booking (mlmapping_amd/csrc/mlm_sector_book.h) on the CPU: tests/cpp/sector_book_driver.cpp, built with
-fsanitize=address,undefined, books random record sets record by record and centre by centre into plain array tables and compares
every field of every entry (first-touch time, kinds, count and strength sum, reference rows, the wrapped flags), and the packed target
lists with the spreads they were made from."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")


def _define(path, name):
    return re.search(r"#define %s (\d+)" % name, open(os.path.join(CSRC, path)).read()).group(1)


def test_header_restates_the_kernels_constants():
    """mlm_sector_book.h restates three constants for the CPU build: each must be the value the kernel's headers have"""
    assert _define("mlm_sector_book.h", "MLM_TIME_SLOTS") == _define("mlm_types.h", "MLM_TIME_SLOTS")
    assert _define("mlm_sector_book.h", "MLM_SEC_CNT_BITS") == _define("mlm_host.h", "MLM_SEC_CNT_BITS")
    assert _define("mlm_sector_book.h", "MLM_BOOK_KIND_BITS") == _define("mlm_kernels_sector.h", "MLM_SEC_KIND_BITS")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sbook") / "sector_book_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "sector_book_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}


def test_centre_wise_booking_equals_record_wise(report):
    assert report["n_sets"] == 400 and report["n_records"] > 100000 and report["n_centres"] > 5000 and report["n_entries"] > 10000
    assert report["n_records"] > 3 * report["n_centres"]  # (several records per centre: what the reduction is for)
    assert report["bad_fields"] == 0


def test_wrapped_reference_counts_flag_the_same_cells(report):
    assert report["n_wrapped"] >= 50 * 5  # (the fifty wrapping sets: the centre and at least four of its targets)
    assert report["bad_flags"] == 0
    assert report["more_flags"] == 0  # (never more flags than record by record: a column gives up no more often)


def test_target_lists(report):
    assert report["n_lists"] == report["n_centres"] and report["n_list_more"] > 100 and report["n_lists"] - report["n_list_more"] > 1000
    assert report["bad_lists"] == 0
