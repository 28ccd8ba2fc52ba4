"""The nearest-obstacle search of mlm_query_nearest on the host (mlmapping_amd/csrc/mlm_nearest.h, the control flow the kernel runs too,
under MapView::nearest of mlm_mapview.h, which answers small batches from the library's host mirror), built for the CPU with
-fsanitize=address,undefined and held byte for byte to the contract written in plain Python integers (tests/nearest_ref.py: every
voxel of the cube, no pruning) over random block dumps with absent and released blocks.  The Python reference itself is held to
properties first."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import nearest_ref as nr
from tests import raywalk_ref as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = (1, 2, 3, 6)
FAR = 20  # block index of the planted blocks: further from the random map than any C here reaches


def random_map(rng, n, nblk=40, span=3, p_occ=0.02, p_unk=0.05, p_infl=0.03, released=0.15):
    """a block dump of random classes: blocks of a (2 span)^3 lattice of block indices around 0, some absent, some released; plus
    planted blocks far away, FREE but for: one obstacle in the first corner cell (FAR, FAR, FAR); pairs of obstacles two cells apart
    along z, y and x in (FAR + 2k, FAR, FAR + 4), k = 0, 1, 2 — the voxel between them sees an exact tie"""
    keys = np.unique(rng.integers(-span, span, size=(nblk, 3)), axis=0).astype(np.int32)
    c = n ** 3
    r = rng.random((len(keys), c))
    occ = np.where(r < p_occ, ord("o"), np.where(r < p_occ + p_unk, ord("u"), ord("f"))).astype(np.uint8)
    infl = np.where(rng.random((len(keys), c)) < p_infl, ord("o"), ord("u")).astype(np.uint8)
    col = (rng.random(len(keys)) < released).astype(np.uint8)
    occ[col.astype(bool), 0] = rng.choice([ord("f"), ord("f"), ord("u"), ord("o")], size=int(col.sum()))
    pk = np.array([[FAR, FAR, FAR]] + [[FAR + 2 * k, FAR, FAR + 4] for k in range(3)], dtype=np.int32)
    pocc = np.full((4, c), ord("f"), dtype=np.uint8)
    pocc[0, 0] = ord("o")
    for k, axis in enumerate((2, 1, 0)):
        for t in (0, 2):
            cell = [1, 1, 1]
            cell[axis] = t
            pocc[1 + k, (cell[2] * n + cell[1]) * n + cell[0]] = ord("o")
    return {"keys": np.concatenate([keys, pk]), "occ": np.concatenate([occ, pocc]), "infl": np.concatenate([infl, np.full((4, c), ord("u"), np.uint8)]),
            "collapsed": np.concatenate([col, np.zeros(4, np.uint8)])}


def points(rng, n, d, C):
    """300 positions: uniform ones; voxel centres (natural ties); voxel faces, edges and corners; the planted ties; positions whose
    ball just excludes the planted obstacle that their cube includes; far away; invalid"""
    lo, hi = -3 * n - 2, 3 * n + 2
    uni = rng.uniform(lo * d, hi * d, size=(120, 3))
    cen = (rng.integers(lo, hi, size=(70, 3)) + 0.5) * d
    k = rng.integers(lo, hi, size=(60, 3)).astype(np.float64)
    k += np.where(rng.random((60, 3)) < 0.35, 0.5, 0.0)  # (some coordinates mid-voxel: faces and edges, not only corners)
    k[:20, 1:] += 0.5  # a face in x for certain
    lat = k * d
    tie = np.array([[(FAR + 2 * j) * n + 1.5, FAR * n + 1.5, (FAR + 4) * n + 1.5] for j in range(3)]) * d
    tie = np.repeat(tie, 4, axis=0)
    ob = np.array([FAR * n, FAR * n, FAR * n])
    offs = [(C, C, 0), (C, 0, C), (0, C, C), (C, C, C), (-C, C, 0), (-C, -C, -C), (0, -C, C), (C, 0, 0), (0, -C, 0), (C - 1, C, 0)]
    excl = (ob - np.array(offs) + 0.5) * d
    far = np.array([[5000000.3, 0.5, 0.5], [0.5, -5000000.0, 2.5], [5000000.0, 5000000.0, 5000000.0], [-5000000.7, 1.0, -5000000.2]]) * d
    u = d / 1024.0
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e300, 0, 0], [0, -1e300, 0], [2.0 ** 40 * u, 0, 0], [0, 0, -(2.0 ** 40 + 1) * u],
                    [2.0 ** 41 * u, np.nan, 0]])
    ok = np.array([[(2.0 ** 40 - 2) * u, 0.5 * d, 0.5 * d], [0.5 * d, -(2.0 ** 40 - 2) * u, 0.5 * d]])  # the largest valid |Q|
    pts = np.concatenate([uni, cen, lat, tie, excl, far, bad, ok])
    pts = np.concatenate([pts, rng.uniform(lo * d, hi * d, size=(300 - len(pts), 3))])
    assert pts.shape == (300, 3)
    return pts


def test_python_reference_has_the_properties():
    """on random maps, for every flag set and C: the answer has O, lies in the ball, no voxel of the cube has a smaller tuple; in an
    empty map with UNKNOWN the answer is the point's own voxel, on a face the one below"""
    rng = np.random.default_rng(4)
    seen = {-1: 0, 0: 0, 1: 0}
    for trial, n in enumerate((4, 5, 7)):
        d = (0.2, 0.25, 0.1)[trial]
        classes = rw.block_classes(random_map(rng, n), n)
        for C in CS:
            pts = points(rng, n, d, C)[::3]
            for f in nr.FLAG_SETS:
                for p in pts:
                    res, _ = nr.nearest(p, d, C, classes, f)
                    seen[nr.check_properties(p, d, C, classes, f, res)] += 1
    assert min(seen.values()) >= 50, seen
    empty = lambda vox: np.full(len(np.asarray(vox).reshape(-1, 3)), nr.UNKNOWN, dtype=np.int64)
    on_face = 0
    for p in points(rng, 5, 0.25, 2):
        Q = rw.lattice(p, 0.25)
        if Q is None:
            continue
        res, _ = nr.nearest(p, 0.25, 2, empty, nr.UNKNOWN)
        want = tuple((q >> 10) - (1 if q % 1024 == 0 else 0) for q in Q)
        on_face += any(q % 1024 == 0 for q in Q)
        assert res[0] == 1 and res[1] == want, (p, res, want)
    assert on_face >= 50
    # by hand: one obstacle at (3, 0, 0), the point at the centre of (0, 0, 0)
    only = lambda vox: np.where((np.asarray(vox).reshape(-1, 3) == [3, 0, 0]).all(axis=1), nr.OCC, 0)
    assert nr.nearest([0.1, 0.1, 0.1], 0.2, 3, only, nr.OCC)[0] == (1, (3, 0, 0), (3072, 0, 0), 9 << 20, nr.dist_of(9 << 20, 0.2))
    assert nr.nearest([0.1, 0.1, 0.1], 0.2, 2, only, nr.OCC)[0] == (0, (0, 0, 0), (0, 0, 0), -1, -1.0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("nearest") / "nearest_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "nearest_driver.cpp"), "-o", str(out)])
    return str(out)


def run_driver(exe, path, d_sub, n, b, pts, cases):
    """cases: [(flags, C)] -> [{"status", "voxel", "delta", "sq", "dist"}]"""
    blob = struct.pack("<d4i", d_sub, n, b["keys"].shape[0], len(pts), len(cases))
    blob += np.array(cases, dtype=np.int32).tobytes()
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    blob += np.ascontiguousarray(pts, dtype=np.float64).tobytes()
    path.write_bytes(blob)
    out = [ln.split() for ln in subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    m = len(pts)
    assert len(out) == m * len(cases)
    res = []
    for k in range(len(cases)):
        rows = out[k * m:(k + 1) * m]
        r = np.array([[int(x) for x in row[:8]] for row in rows], dtype=np.int64).reshape(m, 8)
        res.append({"status": r[:, 0].astype(np.int8), "voxel": r[:, 1:4].astype(np.int32), "delta": r[:, 4:7].astype(np.int32), "sq": r[:, 7].copy(),
                    "dist": np.array([int(row[8], 16) for row in rows], dtype=np.uint64).view(np.float64)})
    return res


def test_host_search_equals_the_reference(exe, tmp_path):
    rng = np.random.default_rng(11)
    status = {-1: 0, 0: 0, 1: 0}
    ties = {0: 0, 1: 0, 2: 0}
    cube_differs = on_lattice = 0
    for trial, n in enumerate((4, 5, 7)):
        d = (0.2, 0.25, 0.1)[trial]
        b = random_map(rng, n)
        classes = rw.block_classes(b, n)
        for C in CS:
            pts = points(rng, n, d, C)
            cases = [(f, C) for f in nr.FLAG_SETS]
            got = run_driver(exe, tmp_path / f"near_{n}_{C}.bin", d, n, b, pts, cases)
            on_lattice += sum(1 for p in pts for Q in [rw.lattice(p, d)] if Q is not None and any(q % 1024 == 0 for q in Q))
            for (f, _), g in zip(cases, got):
                exp, why = nr.nearest_all(pts, d, C, classes, f)
                nr.assert_equal(g, exp, f"n={n} C={C} flags={f}")
                for s in exp["status"]:
                    status[int(s)] += 1
                for w in why:
                    if w["tie"] is not None:
                        ties[w["tie"]] += 1
                    cube_differs += w["cube_differs"]
    # not vacuous: every status, ties resolved on every axis, points a cube rule would answer differently, points on voxel faces
    assert min(status.values()) >= 50, status
    assert min(ties.values()) >= 30, ties
    assert cube_differs >= 30, cube_differs
    assert on_lattice >= 200, on_lattice
