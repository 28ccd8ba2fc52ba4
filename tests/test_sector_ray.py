"""The integer walk of one lane's share of a k_sector ray (mlmapping_amd/csrc/mlm_sector_ray.h) on the CPU, built with
-fsanitize=address,undefined -ffp-contract=off (tests/cpp/sector_ray_driver.cpp) and held to the reference's own sequence
round(z - k * ((z - zc) / rho)) (map_awareness.cpp:266-274, C round), range-clipped: every rho in 2 .. 512, every z, zc for nZ = 41, 81
and 161, four and sixteen lanes per ray.  The union of the lanes' visited (row, cell) sets equals the reference's, in mask mode (steps of
equal row and mask word merged) and in frontier mode (a step per cell, whose time is k - 1); ties — exact half-integers, which only the FP64
sequence decides — must really occur: at least one case in a hundred."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sray") / "sector_ray_driver"
    flags = []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sector_ray_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}


def test_every_ray_is_covered(report):
    assert report["cases"] == 511 * (41 + 81 + 161) * 2
    assert report["steps"] == (41 + 81 + 161) * sum(rho - 1 for rho in range(2, 513))


def test_mask_mode_visits_the_reference_set(report):
    assert report["bad_mask"] == 0 and report["twice"] == 0 and report["visits"] > 0


def test_frontier_mode_times_are_the_steps(report):
    assert report["bad_frontier"] == 0


def test_ties_are_exercised(report):
    assert report["tie_cases"] * 100 >= report["cases"], report
    assert report["tie_steps"] > 0 and report["late_ties"] > 0, report  # (... also in the later pieces of a share longer than 64 steps)
