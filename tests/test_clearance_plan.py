"""The segment walk through a distance field of mlm_query_clearance on the host (mlmapping_amd/csrc/mlm_clearance.h, the control flow the
kernels and the entry point's host branch run too), built for the CPU with -fsanitize=address,undefined and held byte for byte to the
contract written in plain Python integers (tests/clearance_ref.py): arbitrary int32 fields, boxes of one voxel and of odd edges, lo
negative and across 0, segments that start outside, leave, or pass through the outside, zero-length and grazing segments, invalid end
points, sq_stop -1 and >= sq_cap, and groups.  The driver also runs the walk with a look-ahead of 2, 4 and 5 voxels and fails unless
every one gives the bytes of the walk without.  The Python reference itself is held to properties and to a case by hand first."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import raywalk_ref as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 0.2
BOXES = (((0, 0, 0), (1, 1, 1)), ((-2, -1, 0), (5, 3, 2)), ((-3, -2, -4), (8, 4, 4)), ((-7, 2, -1), (13, 9, 6)))  # lo, dims
STOPS = ((-1, 64), (0, 64), (9, 64), (64, 64), (100, 9), (1 << 20, 1 << 20), (3, 1))  # sq_stop, sq_cap
SEED = 77


def centre(v, d=D):
    """positions whose lattice coordinates are exactly the voxel centres 1024 v + 512"""
    Q = np.asarray(v, dtype=np.int64).reshape(-1, 3) * 1024 + 512
    p = (Q + 0.5) * d / 1024.0
    assert all(rw.lattice(x, d) == q for x, q in zip(p, Q.tolist()))
    return p


def by_hand(d=D):
    """an 8 x 4 x 4 field at lo (0, 0, 0), 50 everywhere, 0 at voxel (5, 1, 1), 4 at (4, 1, 1) and 9 at (3, 1, 1); a segment along x
    from voxel (1, 1, 1) to (7, 1, 1)"""
    f = np.full((4, 4, 8), 50, dtype=np.int32)
    f[1, 1, 5], f[1, 1, 4], f[1, 1, 3] = 0, 4, 9
    return (0, 0, 0), (8, 4, 4), f, centre([1, 1, 1], d), centre([7, 1, 1], d)


def test_python_reference_by_hand_and_properties():
    lo, dims, f, a, b = by_hand()
    one = lambda stop, cap, **kw: cr.walk(a[0], b[0], D, lo, dims, f, stop, cap, kw.get("outside_pass", False))
    # stops at the zero voxel: 4 voxels passed (50, 50, 9, 4 clamped to 16), entered at (4 * 1024 - 512) / (6 * 1024)
    assert one(0, 16) == (1, (5, 1, 1), 3584 / 6144, 4, 0, (5, 1, 1), 0 + 0 + 7 + 12, 2)
    # radius 2: stops one voxel earlier, at f = 4
    assert one(4, 16) == (1, (4, 1, 1), 2560 / 6144, 3, 4, (4, 1, 1), 7, 1)
    # nothing stops it: the whole path, minimum 0 at (5, 1, 1), cost 7 + 12 + 16
    assert one(-1, 16) == (0, (7, 1, 1), 1.0, 7, 0, (5, 1, 1), 35, 3)
    # the same segment reversed meets (5, 1, 1) after (7, 1, 1) and (6, 1, 1)
    assert cr.walk(b[0], a[0], D, lo, dims, f, 0, 16, False)[:4] == (1, (5, 1, 1), 1536 / 6144, 2)
    # leaving the box: a segment from (6, 1, 1) to (10, 1, 1) leaves at voxel (8, 1, 1) after two voxels; with OUTSIDE_PASS it runs on
    c, e = centre([6, 1, 1])[0], centre([10, 1, 1])[0]
    assert cr.walk(c, e, D, lo, dims, f, 0, 16, False) == (cr.LEFT, (8, 1, 1), 1536 / 4096, 2, 16, (6, 1, 1), 0, 0)
    assert cr.walk(c, e, D, lo, dims, f, 0, 16, True) == (0, (10, 1, 1), 1.0, 5, 16, (6, 1, 1), 0, 0)
    # starting outside: nothing seen; with OUTSIDE_PASS and sq_stop >= sq_cap the outside voxel itself stops the walk
    assert cr.walk(e, c, D, lo, dims, f, 0, 16, False) == (cr.LEFT, (10, 1, 1), 0.0, 0, cr.NONE, (0, 0, 0), 0, 0)
    assert cr.walk(e, c, D, lo, dims, f, 16, 16, True) == (1, (10, 1, 1), 0.0, 0, 16, (10, 1, 1), 0, 0)
    # invalid
    assert cr.walk([np.nan, 0, 0], c, D, lo, dims, f, 0, 16, False) == (-1, (0, 0, 0), 0.0, 0, cr.NONE, (0, 0, 0), 0, 0)
    # groups: [the by-hand segment stopped], [], [free, stopped, free], [invalid first]; one trailing ray in no group
    p0 = np.concatenate([a, centre([0, 3, 3]), a, centre([0, 0, 0]), [[np.inf, 0, 0]], a, a])
    p1 = np.concatenate([b, centre([7, 3, 3]), b, centre([0, 2, 0]), [[0.0, 0, 0]], b, b])
    res = cr.clearance_all(p0, p1, D, lo, dims, f, 0, 16)
    assert res["status"].tolist() == [1, 0, 1, 0, -1, 1, 1]
    t = cr.group_rows(res, [0, 1, 1, 4, 6])
    assert t.tolist() == [[1, 0, 1, 0, 0, 19, 4, 2], [0, -1, 0, -1, -1, 0, 0, 0], [3, 1, 1, 0, 1, 19, 8 + 4, 2], [2, 0, -1, -1, -1, 0, 0, 0]]
    # properties over random segments: the per-ray relations of the contract
    rng = np.random.default_rng(3)
    lo, dims = (-3, -2, -4), (8, 4, 4)
    fld = cr.wild_field(rng, dims)
    p0, p1 = cr.segments(rng, lo, dims, D, 200)
    for stop, cap in STOPS:
        for op in (False, True):
            r = cr.clearance_all(p0, p1, D, lo, dims, fld, stop, cap, op)
            st = r["status"]
            assert set(np.unique(st)) <= {-1, 0, 1, 2} and (op or stop < 0 or (st == 2).any()) and not (op and (st == 2).any())
            hit = st == 1
            assert (r["min_sq"][hit] <= stop).all() and np.array_equal(r["min"][hit], r["voxel"][hit])
            assert (r["cost"] <= r["n_near"].astype(np.int64) * cap).all() and (r["n_near"] <= r["n_steps"]).all()
            assert ((r["min_sq"] == cr.NONE) == ((r["n_steps"] == 0) & ~hit)).all()
            if stop < 0:
                assert not hit.any()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("clearance") / "clearance_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "clearance_driver.cpp"), "-o", str(out)])
    return str(out)


def run_driver(exe, path, d, p0, p1, lo, dims, field, sq_stop, sq_cap, flags, group_begin=None):
    n = len(p0)
    ng = -1 if group_begin is None else len(group_begin) - 1
    blob = struct.pack("<d5i", d, n, ng, sq_stop, sq_cap, flags) + np.concatenate([lo, dims]).astype(np.int32).tobytes()
    blob += np.ascontiguousarray(p0, dtype=np.float64).tobytes() + np.ascontiguousarray(p1, dtype=np.float64).tobytes()
    if group_begin is not None:
        blob += np.asarray(group_begin, dtype=np.int32).tobytes()
    blob += np.ascontiguousarray(field, dtype=np.int32).tobytes()
    path.write_bytes(blob)
    out = path.with_suffix(".out")
    subprocess.run([exe, str(path), str(out)], check=True)
    raw = out.read_bytes()
    got, at = {}, 0
    for k in cr.OUTPUTS:
        dt, sh = cr.TYPES[k]
        cnt = n * int(np.prod(sh, dtype=np.int64))
        got[k] = np.frombuffer(raw, dtype=dt, count=cnt, offset=at).reshape((n,) + sh)
        at += cnt * np.dtype(dt).itemsize
    if ng >= 0:
        got["table"] = np.frombuffer(raw, dtype=np.int64, count=ng * cr.ROW, offset=at).reshape(ng, cr.ROW)
        at += ng * cr.ROW * 8
    assert at == len(raw)
    return got


def random_groups(rng, n):
    """group_begin with an empty group, single segments, longer runs, and trailing rays in no group"""
    cuts = np.sort(rng.integers(0, n - 3, size=12))
    return np.concatenate([[0, 0, 1], cuts[cuts > 1], [n - 3]]).astype(np.int32)


def test_host_walk_equals_the_reference(exe, tmp_path):
    rng = np.random.default_rng(SEED)
    seen = set()
    for bi, (lo, dims) in enumerate(BOXES):
        field = cr.wild_field(rng, dims)
        p0, p1 = cr.segments(rng, lo, dims, D, 120)
        # (a first segment that is invalid in its group: the group [n - 3 .. ) is not listed; put NaN at the start of a listed one)
        gb = random_groups(rng, len(p0))
        k = next(k for k in range(2, len(gb) - 1) if gb[k + 1] > gb[k])
        p0[gb[k]] = [np.nan, 0.0, 0.0]
        for si, (stop, cap) in enumerate(STOPS):
            for flags in (0, cr.OUTSIDE_PASS):
                exp = cr.clearance_all(p0, p1, D, lo, dims, field, stop, cap, bool(flags))
                exp["table"] = cr.group_rows(exp, gb)
                got = run_driver(exe, tmp_path / f"c_{bi}_{si}_{flags}.bin", D, p0, p1, lo, dims, field, stop, cap, flags, gb)
                cr.assert_equal(got, exp, f"lo={lo} dims={dims} sq_stop={stop} sq_cap={cap} flags={flags}")
                seen |= {int(s) for s in np.unique(exp["status"])}
                assert (exp["table"][:, 0] == 0).any() and (exp["table"][:, 0] == 1).any() and (exp["table"][:, 2] == -1).any()
        # no groups at all
        exp = cr.clearance_all(p0, p1, D, lo, dims, field, 9, 64)
        got = run_driver(exe, tmp_path / f"c_{bi}_plain.bin", D, p0, p1, lo, dims, field, 9, 64, 0)
        assert "table" not in got
        cr.assert_equal(got, exp, f"lo={lo} dims={dims} no groups")
    assert seen == {-1, 0, 1, 2}


def test_by_hand_through_the_driver(exe, tmp_path):
    lo, dims, f, a, b = by_hand()
    got = run_driver(exe, tmp_path / "hand.bin", D, a, b, lo, dims, f, 0, 16, 0, [0, 1])
    assert (int(got["status"][0]), got["voxel"][0].tolist(), float(got["t"][0]), int(got["n_steps"][0]), int(got["min_sq"][0]), got["min"][0].tolist(),
            int(got["cost"][0]), int(got["n_near"][0])) == (1, [5, 1, 1], 3584 / 6144, 4, 0, [5, 1, 1], 19, 2)
    assert got["table"].tolist() == [[1, 0, 1, 0, 0, 19, 4, 2]]


def test_grazed_voxels_are_seen(exe, tmp_path):
    """a diagonal exactly through voxel corners of the plane z = const: the path visits the voxels it grazes (tie to the lowest axis: x
    first), and a zero there stops the walk although the segment only touches its corner"""
    lo, dims = (0, 0, 0), (6, 6, 2)
    f = np.full((2, 6, 6), 30, dtype=np.int32)
    f[0, 1, 2] = 0  # voxel (2, 1, 0): entered by the x step at the corner (2, 2) from (1, 1, 0)
    a, b = np.array([[0.0, 0.0, 0.5 * D]]), np.array([[5 * D, 5 * D, 0.5 * D]])
    pth = [v for v, _ in rw.path(*rw.valid(a[0], b[0], D))[0]]
    assert pth[:4] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0)]
    exp = cr.clearance_all(a, b, D, lo, dims, f, 0, 25)
    assert exp["status"].tolist() == [1] and exp["voxel"].tolist() == [[2, 1, 0]] and exp["n_steps"].tolist() == [3] and exp["t"].tolist() == [0.4]
    cr.assert_equal(run_driver(exe, tmp_path / "graze.bin", D, a, b, lo, dims, f, 0, 25, 0), exp, "grazing")
