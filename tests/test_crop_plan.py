"""mlm_crop_blocks on the CPU: the plan of mlmapping_amd/csrc/mlm_crop.h — argument check, predicate, the hole-filling rule as the device
phases run it (flags, three-phase scan, list, page-out, move by pairs, tail reset), the shrink rule — built with
g++ -fsanitize=address,undefined (tests/cpp/crop_driver.cpp) and held byte for byte to the rule in numpy (tests/crop_ref.py), which is
itself held to the properties the contract states."""
import os
import subprocess

import numpy as np
import pytest

from tests import crop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
NBS = [0, 1, 2, 63, 64, 65, 255, 257, 5000]
PATTERNS = ["none", "all", "first_half", "last_half", "alternating", "random10", "random50", "random90"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("crop")
    exe = d / "crop_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "crop_driver.cpp"), "-o", str(exe)])

    def lines(mode, *cases):
        args = [str(int(v)) for c in cases for v in c]
        return subprocess.run([str(exe), mode, *args], check=True, capture_output=True, text=True).stdout.splitlines()

    def run(blocks, key_lo, key_dims, flags, cap, want_out, seed=1):
        nb, C = blocks["log_odds"].shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([nb, C, *key_lo, *key_dims, flags, cap, int(want_out), seed], dtype=np.int64).tobytes())
            for k, dt in (("keys", np.int32), ("log_odds", np.float32), ("occ", np.uint8), ("infl", np.uint8), ("collapsed", np.uint8)):
                f.write(np.ascontiguousarray(blocks[k], dtype=dt).tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:48], dtype=np.int64)
        at = 48

        def take(rows):
            nonlocal at
            out = {}
            for k, dt, cols in (("keys", np.int32, 3), ("log_odds", np.float32, C), ("occ", np.uint8, C), ("infl", np.uint8, C), ("collapsed", np.uint8, 1)):
                size = rows * cols * np.dtype(dt).itemsize
                out[k] = np.frombuffer(raw[at:at + size], dtype=dt).reshape((rows, cols) if cols > 1 or k == "keys" else (rows,))
                at += size
            return out
        pool = take(nb)
        rows = take(int(head[4]))
        assert at == len(raw)
        return {"status": int(head[0]), "nb": int(head[1]), "K": int(head[2]), "D": int(head[3]), "written": int(head[4]), "H": int(head[5]),
                "pool": pool, "rows": rows}

    return type("Driver", (), {"lines": staticmethod(lines), "run": staticmethod(run)})


def make_blocks(rng, keys, cells):
    """distinct log-odds per voxel, random classes, random released flags"""
    nb = len(keys)
    lo = (np.arange(nb * cells, dtype=np.float32).reshape(nb, cells) * np.float32(0.25) - np.float32(7.0))
    occ = rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(nb, cells))
    infl = rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(nb, cells))
    return {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": lo, "occ": occ, "infl": infl,
            "collapsed": (rng.random(nb) < 0.3).astype(np.uint8)}


def pattern_keys(rng, nb, pattern):
    """keys of nb distinct blocks such that the box x in [0, 1) (INSIDE) drops the slots the pattern names"""
    s = np.arange(nb)
    drop = {"none": np.zeros(nb, bool), "all": np.ones(nb, bool), "first_half": s < nb // 2, "last_half": s >= nb // 2,
            "alternating": s % 2 == 1}.get(pattern)
    if drop is None:
        drop = rng.random(nb) < int(pattern[6:]) / 100.0
    keys = np.stack([np.where(drop, 0, 1 + s % 3), s // 100 - 20, s % 100 - 50], axis=1)
    return keys.astype(np.int32), drop


def same(a, b, rows=None):
    for k in ("keys", "log_odds", "occ", "infl", "collapsed"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if rows is not None:
            x, y = x[:rows], y[:rows]
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def test_python_rule_has_the_properties():
    """the kept blocks are exactly the kept blocks, each once; kept blocks below K do not move; at most min(D, K) move; the dropped come
    out in ascending order of their old slot"""
    rng = np.random.default_rng(5)
    for nb in NBS:
        for pattern in PATTERNS:
            _, drop = pattern_keys(rng, nb, pattern)
            p = ref.plan(drop)
            assert p["D"] == int(drop.sum()) and p["K"] == nb - p["D"] and p["H"] == int(drop[:p["K"]].sum())
            assert sorted(p["order"].tolist()) == np.flatnonzero(~drop).tolist()
            stay = np.flatnonzero(~drop[:p["K"]])
            assert np.array_equal(p["order"][stay], stay)
            assert int((p["order"] != np.arange(p["K"])).sum()) == p["H"] <= min(p["D"], p["K"])
            assert np.array_equal(p["rows"], np.flatnonzero(drop))
            moved = p["order"][np.flatnonzero(drop[:p["K"]])]
            assert np.all(moved >= p["K"]) and np.all(np.diff(moved) > 0)


@pytest.mark.parametrize("nb", NBS)
def test_driver_matches_the_rule(driver, nb):
    rng = np.random.default_rng(100 + nb)
    for cells in (8, 27):
        for pattern in PATTERNS:
            keys, drop = pattern_keys(rng, nb, pattern)
            blocks = make_blocks(rng, keys, cells)
            for want_out in (False, True):
                got = driver.run(blocks, [0, -(1 << 20), -(1 << 20)], [1, 1 << 21, 1 << 21], ref.INSIDE, nb, want_out, seed=nb + cells)
                kept, rows, p = ref.crop(blocks, [0, -(1 << 20), -(1 << 20)], [1, 1 << 21, 1 << 21], True)
                assert np.array_equal(ref.drops(keys, [0, -(1 << 20), -(1 << 20)], [1, 1 << 21, 1 << 21], True), drop)
                assert (got["status"], got["nb"], got["K"], got["D"], got["H"]) == (0, nb, p["K"], p["D"], p["H"]), (pattern, cells)
                same(got["pool"], kept, rows=p["K"])
                tail = {k: v[p["K"]:] for k, v in got["pool"].items()}
                if p["D"]:
                    assert not tail["log_odds"].any() and np.all(tail["occ"] == ord("u")) and np.all(tail["infl"] == ord("u")) and not tail["collapsed"].any()
                assert got["written"] == (p["D"] if want_out else 0)
                if want_out:
                    same(got["rows"], rows)


def test_predicates_key_range_and_int32_edges(driver):
    rng = np.random.default_rng(9)
    keys = np.concatenate([rng.integers(-4, 4, size=(300, 3)),
                           [[ref.KEY_MIN] * 3, [ref.KEY_MAX] * 3, [ref.KEY_MIN, 0, ref.KEY_MAX], [ref.KEY_MAX, ref.KEY_MIN, 0]]])
    keys = np.unique(keys, axis=0).astype(np.int32)
    keys = keys[rng.permutation(len(keys))]
    blocks = make_blocks(rng, keys, 8)
    boxes = [([-2, -2, -2], [4, 4, 4]), ([0, 0, 0], [1, 1, 1]), ([-4, -4, 1], [8, 8, 1]),
             ([ref.KEY_MIN] * 3, [1 << 21] * 3), ([ref.KEY_MAX] * 3, [1, 1, 1]), ([ref.KEY_MIN] * 3, [1, 1, 1]),
             ([ref.I32_MIN] * 3, [ref.I32_MAX] * 3), ([0, 0, 0], [ref.I32_MAX] * 3), ([ref.I32_MAX - 1] * 3, [1, 1, 1]),
             ([ref.I32_MIN] * 3, [1, 1, 1]), ([ref.I32_MIN, -1, -1], [ref.I32_MAX, 3, 3])]
    seen = set()
    for lo, dims in boxes:
        for inside in (False, True):
            got = driver.run(blocks, lo, dims, ref.INSIDE if inside else ref.OUTSIDE, len(keys), True)
            kept, rows, p = ref.crop(blocks, lo, dims, inside)
            assert (got["status"], got["K"], got["D"], got["H"]) == (0, p["K"], p["D"], p["H"]), (lo, dims, inside)
            same(got["pool"], kept, rows=p["K"])
            same(got["rows"], rows)
            seen.add((p["D"] == 0, p["K"] == 0))
    assert seen == {(True, False), (False, True), (False, False)}


def test_dry_and_capacity_leave_the_pool_alone(driver):
    rng = np.random.default_rng(2)
    keys, drop = pattern_keys(rng, 257, "random50")
    blocks = make_blocks(rng, keys, 27)
    D = int(drop.sum())
    box = ([0, -(1 << 20), -(1 << 20)], [1, 1 << 21, 1 << 21])
    for flags, cap, want_out, status in ((ref.INSIDE | ref.DRY, D, True, 0), (ref.INSIDE | ref.DRY, 0, False, 0), (ref.INSIDE, D - 1, True, ref.ERR_CAPACITY),
                                         (ref.INSIDE, 0, True, ref.ERR_CAPACITY)):
        got = driver.run(blocks, *box, flags, cap, want_out)
        assert (got["status"], got["D"], got["K"], got["written"]) == (status, D, 257 - D, 0)
        same(got["pool"], blocks)
    got = driver.run(blocks, *box, ref.INSIDE, 0, False)  # no outputs: cap is ignored
    assert (got["status"], got["K"], got["written"]) == (0, 257 - D, 0)


INVALID = [((0, 0, 0, 0, 1, 1, 1, 0, 0), 1),                                   # no box
           ((1, 0, 0, 0, 0, 1, 1, 0, 0), 2), ((1, 0, 0, 0, 1, -1, 1, 0, 0), 2), ((1, 0, 0, 0, 1, 1, ref.I32_MIN, 0, 0), 2),
           ((1, ref.I32_MAX, 0, 0, 1, 1, 1, 0, 0), 3), ((1, 0, 1, 0, 1, ref.I32_MAX, 1, 0, 0), 3), ((1, 0, 0, 2, 1, 1, ref.I32_MAX - 1, 1, 0), 3),
           ((1, 0, 0, 0, 1, 1, 1, 8, 0), 4), ((1, 0, 0, 0, 1, 1, 1, -1, 0), 4), ((1, 0, 0, 0, 1, 1, 1, 16 | 1, 0), 4),
           ((1, 0, 0, 0, 1, 1, 1, 0, -1), 5), ((1, 0, 0, 0, 1, 1, 1, 7, ref.I32_MIN), 5)]
VALID = [(1, 0, 0, 0, 1, 1, 1, 0, 0), (1, ref.I32_MAX - 1, 0, 0, 1, 1, 1, 7, 5), (1, ref.I32_MIN, ref.I32_MIN, ref.I32_MIN, ref.I32_MAX, ref.I32_MAX, ref.I32_MAX, 1, ref.I32_MAX),
         (1, 0, 0, 0, ref.I32_MAX, 1, 1, 2, 0), (1, -5, 7, 9, 3, 2, 1, 4, 1)]


def test_argument_check(driver):
    out = driver.lines("args", *[c for c, _ in INVALID], *VALID)
    codes = [int(line.split()[0]) for line in out]
    assert codes == [code for _, code in INVALID] + [0] * len(VALID)
    for (c, code), line in zip(INVALID, out):
        assert len(line.split(None, 1)[1]) > 5
        lo, dims = (None, None) if not c[0] else (c[1:4], c[4:7])
        assert ref.check_args(lo, dims, c[7], c[8]) == code
    for c in VALID:
        assert ref.check_args(c[1:4], c[4:7], c[7], c[8]) == 0


def test_shrink_rule(driver):
    cases = [(c0, cap, K) for c0 in (1, 3, 64, 1000, 4096) for cap in (c0, 2 * c0, 3 * c0, 8 * c0, 8 * c0 + 5, 1 << 28)
             for K in (0, 1, c0 // 2, c0 // 2 + 1, c0, c0 + 1, 2 * c0, 2 * c0 + 1, 4 * c0 - 1, 4 * c0, cap // 2, cap)]
    got = [int(v) for v in driver.lines("shrink", *cases)]
    assert got == [ref.shrink_target(*c) for c in cases]
    for (c0, cap, K), t in zip(cases, got):
        if t:
            k = (t // c0).bit_length() - 1
            assert t == c0 << k and t >= max(c0, 2 * K) and t < cap and (k == 0 or t // 2 < max(c0, 2 * K))
        else:
            t2 = c0
            while t2 < max(c0, 2 * K):
                t2 *= 2
            assert t2 >= cap
    assert sum(1 for t in got if t) > 40 and sum(1 for t in got if not t) > 40


def test_lane_widths(driver):
    """16 bytes per lane where a block's rows are 16-byte aligned, else a dword, else a byte (subbox_n 2 .. 16)"""
    ns = [2, 3, 4, 5, 7, 8, 10, 16]
    got = [tuple(int(v) for v in line.split()) for line in driver.lines("widths", *[[n ** 3] for n in ns])]
    assert got == [(16, 4), (4, 1), (16, 16), (4, 1), (4, 1), (16, 16), (16, 4), (16, 16)]
    for n, (fw, bw) in zip(ns, got):
        assert (n ** 3 * 4) % fw == 0 and (n ** 3) % bw == 0


def test_binding_names_the_call():
    from mlmapping_amd import mlmap

    assert "mlm_crop_blocks" in mlmap.ABI_SYMBOLS
    assert (mlmap.MLM_CROP_OUTSIDE, mlmap.MLM_CROP_INSIDE, mlmap.MLM_CROP_DRY, mlmap.MLM_CROP_SHRINK, mlmap.MLM_CROP_ROW) == \
        (ref.OUTSIDE, ref.INSIDE, ref.DRY, ref.SHRINK, ref.ROW)
    assert hasattr(mlmap.MLMap, "crop_blocks") and hasattr(mlmap.MLMap, "retain_around")
    lo, dims = ref.retain_box([1.0, -2.5, 0.3], 3.0, 1.0)
    assert lo.tolist() == [-3, -7, -4] and dims.tolist() == [9, 9, 9]
