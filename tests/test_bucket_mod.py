"""MlmBktMod (mlmapping_amd/csrc/mlm_host.h): k_sector takes the bucket of a hit — the sign-extended 32-bit hash code modulo the emulated
container's bucket count — as a 32-bit remainder by a host-made multiplier (non-negative codes) or from 2^64 mod n and the remainder of
the negated code (negative codes) instead of a 64-bit remainder.  Both forms have to be exact for every one of the 2^32 codes and every
bucket count below 2^32; larger counts must keep the 64-bit remainder.  The driver checks them against unsigned __int128 arithmetic:
exhaustively for four divisors, and on 2^16 strided codes plus the edge codes for every bucket count libstdc++ can choose."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bm") / "bucket_mod_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "bucket_mod_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}


def test_both_forms_exact_for_all_codes(report):
    """divisors 2, 3, 4 294 967 291 and 20 753 (a config-2 stream's bucket count): all 2^32 codes, non-negative and negative"""
    assert report["checked"] == 4 << 32 and report["bad"] == 0


def test_both_forms_exact_for_every_bucket_count_of_libstdcxx(report):
    assert report["primes"] >= 200  # (the list has 256 entries below 2^32 on LP64)
    assert report["prime_checked"] == report["primes"] * ((1 << 16) + 5) and report["prime_bad"] == 0
    assert report["c_bad"] == 0  # (2^64 mod n as the host makes it)
    assert report["one"] == 1    # (a container of one bucket)


def test_bucket_counts_of_two_to_the_32_or_more_keep_the_64_bit_remainder(report):
    assert report["first_big"] >= 1 << 32 and report["fallback"] == 3
