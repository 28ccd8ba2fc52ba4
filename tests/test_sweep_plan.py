"""The swept ball of mlm_query_sweeps on the host (mlmapping_amd/csrc/mlm_sweep.h, the control flow the kernel runs too, under
MapView::sweep of mlm_mapview.h, which answers small batches from the library's host mirror), built for the CPU with
-fsanitize=address,undefined and held byte for byte to the contract written in plain Python integers (tests/sweep_ref.py: the full ball
at every path voxel, no caps) over random block dumps with absent and released blocks.  The Python reference itself is held to
properties first."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import raywalk_ref as rw
from tests import sweep_ref as sr
from tests.test_nearest_plan import FAR, random_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (0, 1, 2, 3, 5, 16)
GEOMETRIES = ((4, 0.2, 150), (5, 0.25, 120), (7, 0.1, 80), (10, 0.2, 40))  # n, d, blocks drawn: about as many obstacle voxels in each
N_UNIFORM = 120
LONG = 30  # radius 16 only on rays of at most this many voxels: the reference tests 17 077 voxels per path voxel


def centre(v, d):
    return (np.asarray(v, dtype=np.float64).reshape(-1, 3) + 0.5) * d


def planted_rays(n, d):
    """rays that run into the planted obstacle pairs of random_map between the two obstacles, perpendicular to the pair: both enter the
    ball in the same step at the same distance and differ in z, in y, in x in turn; 21 voxels each"""
    a, b = [], []
    for k, along in enumerate((0, 2, 1)):  # the pair along z is approached along x, the one along y along z, the one along x along y
        mid = np.array([(FAR + 2 * k) * n + 1, FAR * n + 1, (FAR + 4) * n + 1])
        start = mid.copy()
        start[along] -= 20
        a.append(start), b.append(mid)
    return centre(a, d), centre(b, d)


def rays_of(rng, n, d):
    lo, hi = (-3 * n - 2) * d, (3 * n + 2) * d
    u0, u1 = rw.uniform_rays(rng, lo, hi, N_UNIFORM, short=8 * d)
    s0, s1 = rw.special_rays(rng, lo, hi, d, count=12)
    w0, w1 = rw.weird_rays(d)
    t0, t1 = planted_rays(n, d)
    return np.concatenate([u0, s0, w0, t0]), np.concatenate([u1, s1, w1, t1])


def test_python_reference_has_the_properties():
    """r = 0 equals raywalk_ref.cast; a stopped ray's hit has O, lies in the ball and no ball voxel has a smaller tuple; no earlier
    path voxel is blocked; one obstacle by hand"""
    rng = np.random.default_rng(3)
    seen = {-1: 0, 0: 0, 1: 0}
    for n, d in ((4, 0.2), (5, 0.25)):
        classes = rw.block_classes(random_map(rng, n, p_occ=0.004), n)
        lo, hi = (-3 * n - 2) * d, (3 * n + 2) * d
        p0, p1 = rw.uniform_rays(rng, lo, hi, 40, short=8 * d)
        w0, w1 = rw.weird_rays(d)
        p0, p1 = np.concatenate([p0, w0[:7]]), np.concatenate([p1, w1[:7]])
        for i in range(len(p0)):
            exp, _ = rw.cast(p0[i], p1[i], d, classes)
            got, _ = sr.sweep(p0[i], p1[i], d, 0, classes)
            for f in sr.FLAG_SETS:
                assert got[f][:5] == exp[f]
                assert got[f][5:] == ((got[f][1], 0) if got[f][0] == 1 else (got[f][1], sr.NONE))
        for r in (1, 2, 3):
            for i in range(0, len(p0), 2):
                got, _ = sr.sweep(p0[i], p1[i], d, r, classes)
                for f in (sr.OCC, sr.OCC | sr.INFL, sr.OCC | sr.INFL | sr.UNKNOWN):
                    seen[sr.check_properties(p0[i], p1[i], d, r, classes, f, got[f])] += 1
    assert min(seen.values()) >= 10, seen
    only = lambda vox: np.where((np.asarray(vox).reshape(-1, 3) == [6, 3, 0]).all(axis=1), sr.OCC, 0)
    a, b = centre([0, 0, 0], 0.2)[0], centre([12, 0, 0], 0.2)[0]
    span = rw.lattice(b, 0.2)[0] - rw.lattice(a, 0.2)[0]  # (voxel 6 is entered 5.5 voxels from the start)
    assert sr.sweep(a, b, 0.2, 3, only, (sr.OCC,))[0][sr.OCC] == (1, (6, 0, 0), 5632 / span, 6, 0, (6, 3, 0), 9)
    assert sr.sweep(a, b, 0.2, 2, only, (sr.OCC,))[0][sr.OCC] == (0, (12, 0, 0), 1.0, 13, 0, (12, 0, 0), sr.NONE)
    assert [sr.columns(r) for r in (0, 1, 2, 4, 5, 8, 16)] == [1, 5, 13, 49, 81, 197, 797]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("sweep") / "sweep_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sweep_driver.cpp"), "-o", str(out)])
    return str(out)


def run_driver(exe, path, d_sub, n, b, p0, p1, cases):
    """cases: [(flags, radius)] -> [{name: array}]"""
    blob = struct.pack("<d4i", d_sub, n, b["keys"].shape[0], len(p0), len(cases))
    blob += np.array(cases, dtype=np.int32).tobytes()
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    blob += np.ascontiguousarray(p0, dtype=np.float64).tobytes() + np.ascontiguousarray(p1, dtype=np.float64).tobytes()
    path.write_bytes(blob)
    out = [ln.split() for ln in subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    m = len(p0)
    assert len(out) == m * len(cases)
    res = []
    for k in range(len(cases)):
        rows = out[k * m:(k + 1) * m]
        r = np.array([[int(x) for x in row[:4] + row[5:]] for row in rows], dtype=np.int64).reshape(m, 10)
        res.append({"status": r[:, 0].astype(np.int8), "voxel": r[:, 1:4].astype(np.int32), "n_steps": r[:, 4].astype(np.int32),
                    "n_unknown": r[:, 5].astype(np.int32), "hit": r[:, 6:9].astype(np.int32), "hit_sq": r[:, 9].astype(np.int32),
                    "t": np.array([int(row[4], 16) for row in rows], dtype=np.uint64).view(np.float64)})
    return res


def test_host_sweep_equals_the_reference(exe, tmp_path):
    rng = np.random.default_rng(12)
    status = {-1: 0, 0: 0, 1: 0}
    ties = {0: 0, 1: 0, 2: 0}
    at_start = 0
    for n, d, nblk in GEOMETRIES:
        b = random_map(rng, n, nblk=nblk, p_occ=0.004)
        classes = rw.block_classes(b, n)
        p0, p1 = rays_of(rng, n, d)
        short = np.array([sr.path_len(a, c, d) <= LONG for a, c in zip(p0, p1)])
        assert short[:N_UNIFORM].sum() >= N_UNIFORM // 4 and short[-3:].all()
        for r in RADII:
            a, c = (p0[short], p1[short]) if r == 16 else (p0, p1)
            cases = [(f, r) for f in sr.FLAG_SETS]
            got = run_driver(exe, tmp_path / f"sweep_{n}_{r}.bin", d, n, b, a, c, cases)
            exp, tie = sr.sweep_all(a, c, d, r, classes)
            for (f, _), g in zip(cases, got):
                sr.assert_equal(g, exp[f], f"n={n} r={r} flags={f}")
                for s in exp[f]["status"]:
                    status[int(s)] += 1
                at_start += int(((exp[f]["status"] == 1) & (exp[f]["n_steps"] == 0)).sum())
                for w in tie[f][-3:]:  # the planted pairs
                    if w is not None:
                        ties[w] += 1
            if r in (2, 3):  # not vacuous: free rays, and rays stopped on their way by an obstacle beside the path
                e = exp[sr.OCC]
                st, k, sq = e["status"][:N_UNIFORM], e["n_steps"][:N_UNIFORM], e["hit_sq"][:N_UNIFORM]
                print(f"n={n} r={r}: not stopped {(st == 0).sum()}, stopped at k > 0 off-centre {((st == 1) & (k > 0) & (sq > 0)).sum()}")
                assert (st == 0).sum() >= N_UNIFORM // 10 and ((st == 1) & (k > 0) & (sq > 0)).sum() >= N_UNIFORM // 10, \
                    (n, r, (st == 0).sum(), ((st == 1) & (k > 0) & (sq > 0)).sum())
    assert min(status.values()) >= 50, status
    assert min(ties.values()) >= 10, ties
    assert at_start >= 20, at_start
