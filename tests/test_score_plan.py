"""The scan-to-map score of mlm_score_poses on the host (mlmapping_amd/csrc/mlm_score.h, the arithmetic the kernel runs too, under
MapView::score of mlm_mapview.h, which answers small batches), built for the CPU with -fsanitize=address,undefined and held byte for
byte to the contract written in numpy (tests/score_ref.py) over random block dumps with absent and released blocks, with unsigned,
signed and arbitrary int32 fields.  The Python reference itself is held to properties first."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import esdf_ref as er
from tests import raywalk_ref as rw
from tests import score_ref as sc
from tests.test_nearest_plan import random_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ((4, 0.2, 150), (5, 0.25, 120), (7, 0.1, 80), (10, 0.2, 40))  # n, d, blocks drawn
N_PTS, N_POSES = 333, 70
CAPS = (1, 64, 1 << 20)
C_FIELD = 8  # max_dist of the two distance fields
SEED = 31


def box_of(n):
    return np.full(3, -2 * n, dtype=np.int64), np.array([4 * n + 3, 4 * n + 1, 3 * n + 2], dtype=np.int64)


def box_voxels(lo, dims):
    iz, iy, ix = np.unravel_index(np.arange(int(np.prod(dims))), (dims[2], dims[1], dims[0]))
    return np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)


def esdf_field(classes, lo, dims, C, signed):
    """mlm_export_esdf's sqdist over the box (OCC), from the classes of the box grown by C"""
    glo, gd = er.grown(list(lo), list(dims), C)
    mask = ((classes(box_voxels(glo, gd)) & sc.OCC) != 0).reshape(gd[2], gd[1], gd[0])
    return np.ascontiguousarray(er.expected(mask, C, signed, 1.0)["sqdist"], dtype=np.int32)


def fields_of(rng, classes, lo, dims):
    wild = rng.integers(-(1 << 31), 1 << 31, size=(int(dims[2]), int(dims[1]), int(dims[0])), dtype=np.int64).astype(np.int32)
    wild.reshape(-1)[:4] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0, -1]
    small = rng.random(wild.shape) < 0.5  # half of it in the range a cap of 64 does not clamp
    wild[small] = rng.integers(-3, 70, size=int(small.sum()))
    return [esdf_field(classes, lo, dims, C_FIELD, False), esdf_field(classes, lo, dims, C_FIELD, True), wild]


def scan_of(rng, n, d):
    ext = (3 * n + 2) * d
    pts = rng.uniform(-0.6 * ext, 0.6 * ext, size=(N_PTS, 3))
    T = np.concatenate([sc.random_rotations(rng, N_POSES), rng.uniform(-0.5 * ext, 0.5 * ext, size=(N_POSES, 3))], axis=1)
    return pts, T


def test_python_reference_has_the_properties():
    rng = np.random.default_rng(5)
    n, d = 5, 0.25
    b = random_map(rng, n)
    classes = rw.block_classes(b, n)
    lo, dims = box_of(n)
    unsigned, signed, wild = fields_of(rng, classes, lo, dims)
    pts, T = scan_of(rng, n, d)
    for f in (unsigned, signed, wild):
        t = sc.score(pts, T, d, classes, (lo, dims), f, 64)
        assert np.array_equal(t[:, 1] + t[:, 2] + t[:, 3], t[:, 0]) and (t[:, 0] == N_PTS).all()
        assert (t[:, 5] <= t[:, 0]).all() and (t[:, 7] <= t[:, 5]).all() and (t[:, 6] <= 64 * t[:, 0]).all()
    # the identity pose and points on voxel centres: [6] is the sum of the clamped field at those voxels
    vox = rng.integers(lo - 2, lo + dims + 2, size=(200, 3))
    cen = (vox + 0.5) * d
    inside = ((vox >= lo) & (vox < lo + dims)).all(axis=1)
    assert 20 <= inside.sum() <= 180
    r = vox - lo
    for f, cap in ((unsigned, 64), (signed, 9), (wild, 1 << 20)):
        want = np.where(inside, np.clip(f.astype(np.int64)[np.where(inside, r[:, 2], 0), np.where(inside, r[:, 1], 0), np.where(inside, r[:, 0], 0)], 0, cap), cap)
        t = sc.score(cen, sc.IDENTITY, d, classes, (lo, dims), f, cap)
        assert t[0, 6] == want.sum() and t[0, 5] == inside.sum() and t[0, 0] == 200
        bits = classes(vox)
        assert t[0, 1:5].tolist() == [((bits & 1) != 0).sum(), ((bits & 5) == 0).sum(), ((bits & 4) != 0).sum(), ((bits & 2) != 0).sum()]
    # a point exactly on a face k * d belongs to voxel k, the next double below it to voxel k - 1, also for negative k.  With a dyadic
    # d the product k * d is the face itself.  Otherwise the double k * d is only the face's neighbour (-29 * 0.2 rounds to
    # -5.800000000000001, which the lattice's own division puts into voxel -30): there the face is the least double the lattice
    # assigns to voxel k, it lies within one ulp of k * d, and the same two statements hold for it.
    ks = np.arange(-40, 41)
    for dd in (0.25, 0.125, 0.2, 0.1):
        x = ks * dd
        vox_x = lambda xs: sc.voxels(sc.world(np.stack([xs, np.full(len(ks), 0.5 * dd), np.full(len(ks), 0.5 * dd)], axis=1), sc.IDENTITY), dd)[1][0, :, 0]
        if dd in (0.25, 0.125):
            face = x
        else:
            cand = np.stack([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])
            ok = np.stack([vox_x(c) >= ks for c in cand])
            assert ok[2].all() and not ok.all(axis=0).all()
            face = cand[np.argmax(ok, axis=0), np.arange(len(ks))]  # the least of the three that has reached voxel k
        assert np.array_equal(vox_x(face), ks) and np.array_equal(vox_x(np.nextafter(face, -np.inf)), ks - 1), dd
    # invalid pairs: a bad point is invalid under every pose, a bad pose has an all-zero row
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e300, 0, 0]])
    t = sc.score(np.concatenate([pts[:10], bad]), T, d, classes, (lo, dims), unsigned, 64)
    assert (t[:, 0] == 10).all() and np.array_equal(t, sc.score(pts[:10], T, d, classes, (lo, dims), unsigned, 64))
    Tb = np.tile(T[:1], (5, 1))
    Tb[1, 4], Tb[2, 9], Tb[3, 11], Tb[4, 10] = np.nan, np.inf, -np.inf, 1e300
    t = sc.score(pts, Tb, d, classes, (lo, dims), unsigned, 64)
    assert t[0, 0] == N_PTS and not t[1:].any()
    # by hand: d = 0.2, one occupied voxel (3, 0, 0); two points, the pose a quarter turn about z plus (0.1, 0.1, 0.1):
    # s = (0, -0.6, 0) -> w = (0.7, 0.1, 0.1): voxel (3, 0, 0); s = (0.2, 0, 0.4) -> w = (0.1, 0.3, 0.5): voxel (0, 1, 2)
    only = lambda vx: np.where((np.asarray(vx).reshape(-1, 3) == [3, 0, 0]).all(axis=1), sc.OCC | sc.INFL, 0)
    quarter = np.array([0.0, -1, 0, 1, 0, 0, 0, 0, 1, 0.1, 0.1, 0.1])
    f = np.full((3, 2, 4), 50, dtype=np.int32)  # box lo (0, 0, 0), dims (4, 2, 3)
    f[0, 0, 3] = -4
    f[2, 1, 0] = 7
    t = sc.score([[0, -0.6, 0], [0.2, 0, 0.4]], quarter, 0.2, only, ([0, 0, 0], [4, 2, 3]), f, 9)
    assert t.tolist() == [[2, 1, 1, 0, 1, 2, 7, 1]]
    t = sc.score([[0, -0.6, 0], [0.2, 0, 0.4]], quarter, 0.2, only, ([0, 0, 0], [4, 1, 3]), f[:, :1, :], 9)
    assert t.tolist() == [[2, 1, 1, 0, 1, 1, 9, 1]]  # ((0, 1, 2) has left the box: sq_cap)
    assert sc.best_row([[5, 1, 0, 0, 0, 0, 9, 0], [5, 3, 0, 0, 0, 0, 7, 0], [5, 4, 0, 0, 0, 0, 7, 0], [5, 4, 0, 0, 0, 0, 7, 0]]) == 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("score") / "score_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "score_driver.cpp"), "-o", str(out)])
    return str(out)


def run_driver(exe, path, d_sub, n, b, pts, T, lo, dims, fields, cases):
    """cases: [(classes, field index or -1, sq_cap)] -> [table int64 [n_poses][8]]"""
    blob = struct.pack("<d6i", d_sub, n, b["keys"].shape[0], len(pts), len(T), len(fields), len(cases))
    blob += np.concatenate([lo, dims]).astype(np.int32).tobytes() + np.array(cases, dtype=np.int32).tobytes()
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    blob += np.ascontiguousarray(pts, dtype=np.float64).tobytes() + np.ascontiguousarray(T, dtype=np.float64).tobytes()
    blob += b"".join(np.ascontiguousarray(f, dtype=np.int32).tobytes() for f in fields)
    path.write_bytes(blob)
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout
    rows = np.array(out.split(), dtype=np.int64).reshape(len(cases), len(T), sc.ROW)
    return [rows[k] for k in range(len(cases))]


def test_host_score_equals_the_reference(exe, tmp_path):
    rng = np.random.default_rng(SEED)
    for n, d, nblk in GEOMETRIES:
        b = random_map(rng, n, nblk=nblk, p_occ=0.02)
        classes = rw.block_classes(b, n)
        lo, dims = box_of(n)
        fields = fields_of(rng, classes, lo, dims)
        pts, T = scan_of(rng, n, d)
        # (a few invalid pairs ride along: two bad points, one bad pose)
        pts = np.concatenate([pts, [[np.nan, 0.0, 0.0], [0.0, 1e300, 0.0]]])
        T = np.concatenate([T, T[:1]])
        T[-1, 9] = np.inf
        tot = sc.non_vacuous(sc.score(pts, T[:N_POSES], d, classes, (lo, dims), fields[0], 64), f"n={n}")
        print(f"n={n} d={d}: [1] {tot[1]} [2] {tot[2]} [3] {tot[3]} [4] {tot[4]} [5] / [0] {tot[5]} / {tot[0]}")
        cases = [(1, -1, 1)] + [(c, fi, cap) for fi in range(3) for cap in CAPS for c in (1, 0)]
        got = run_driver(exe, tmp_path / f"score_{n}.bin", d, n, b, pts, T, lo, dims, fields, cases)
        for (c, fi, cap), g in zip(cases, got):
            exp = sc.score(pts, T, d, classes if c else None, (lo, dims) if fi >= 0 else None, fields[fi] if fi >= 0 else None, cap)
            sc.assert_equal(g, exp, f"n={n} classes={c} field={fi} sq_cap={cap}")
            assert not exp[-1].any() and (exp[:-1, 0] == N_PTS).all()
