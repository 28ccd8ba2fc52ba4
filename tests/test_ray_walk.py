"""The segment casts of mlm_query_rays on the host (mlmapping_amd/csrc/mlm_raywalk.h, the integer walk the kernel runs too, under
MapView::ray of mlm_mapview.h, which answers small batches from the library's host mirror), built for the CPU with
-fsanitize=address,undefined and held to a walk written here in plain Python integers and rationals (tests/raywalk_ref.py) over the
oracle's voxel classes: every output of every flag set, integers exactly, t by its 64 bits.  The Python walk itself is held to
geometry first."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1, SDEF
from tests import raywalk_ref as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_walk_against_geometry():
    """for 4 000 lattice rays (many through exact faces, edges and corners): every visited voxel's closed cube meets the closed
    segment (exact rationals), consecutive voxels differ by one on one axis, the path has N + 1 voxels and ends at floor(Q1 / 1024),
    t is non-decreasing and at most 1"""
    rnd = random.Random(1)
    tie_rays = 0
    for _ in range(4000):
        k = rnd.choice([1, 1, 1024, 512])
        Q0 = [rnd.randint(-40, 40) * k + rnd.choice([0, 0, rnd.randint(-3, 3)]) for _ in range(3)]
        L = rnd.choice([3, 40, 500])
        Q1 = [Q0[a] + rnd.choice([0, 1, -1, 1]) * rnd.randint(0, L) * k for a in range(3)]
        tie_rays += rw.check_geometry(Q0, Q1) > 0
    assert tie_rays >= 300
    # ... and for rays given as positions, the generators' special cases included
    rng = np.random.default_rng(5)
    d = 0.1
    p0, p1 = rw.special_rays(rng, np.array([-3.0, -2.0, -1.0]), np.array([3.0, 2.0, 1.5]), d, count=60)
    w0, w1 = rw.weird_rays(d)
    n_valid = 0
    for a, b in zip(np.concatenate([p0, w0]), np.concatenate([p1, w1])):
        Q = rw.valid(a, b, d)
        if Q is not None and max(abs(Q[1][i] - Q[0][i]) for i in range(3)) < 2 ** 20:  # (the 32 768-voxel rays: too long for rationals per voxel)
            rw.check_geometry(*Q)
            n_valid += 1
    assert n_valid >= 500


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("rays") / "ray_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ray_driver.cpp"), "-o", str(out)])
    return str(out)


def run_driver(exe, path, cfg, b, p0, p1, flag_sets=rw.FLAG_SETS):
    blob = struct.pack("<d4i", cfg.subbox_d_xyz, cfg.subbox_n, b["keys"].shape[0], p0.shape[0], len(flag_sets))
    blob += np.array(flag_sets, dtype=np.int32).tobytes()
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    blob += np.ascontiguousarray(p0, dtype=np.float64).tobytes() + np.ascontiguousarray(p1, dtype=np.float64).tobytes()
    path.write_bytes(blob)
    rows = [ln.split() for ln in subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    n = p0.shape[0]
    assert len(rows) == n * len(flag_sets)
    out = {}
    for k, f in enumerate(flag_sets):
        r = rows[k * n:(k + 1) * n]
        out[f] = {"status": np.array([int(x[0]) for x in r], dtype=np.int8), "voxel": np.array([[int(v) for v in x[1:4]] for x in r], dtype=np.int32),
                  "t": np.array([float.fromhex(x[4]) for x in r], dtype=np.float64), "n_steps": np.array([int(x[5]) for x in r], dtype=np.int32),
                  "n_unknown": np.array([int(x[6]) for x in r], dtype=np.int32)}
    return out


N_RANDOM = 3000


@pytest.mark.parametrize("name", ["SDEF", "S1 frontier n5 (released blocks)"])
def test_host_rays_equal_the_python_walk(exe, tmp_path, name):
    from oracle.binding import OracleMap

    released = "released" in name
    cfg = SDEF.with_(depth_noise_coe=0.00375, lm_occupied_sh=2.0) if not released else S1.with_(use_exploration_frontiers=True, subbox_n=5)
    cpu = OracleMap(cfg)
    shift = np.array([-8.0, -7.5, 0.0])
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 4):
        cpu.update_depth(img, q, np.array(t) + shift)  # (a map in negative x, y; frontier bookkeeping and inflation need z in [0, 5))
    b = cpu.export_blocks()
    full = (b["occ"] == ord("o")).any(axis=1) & ~b["collapsed"].astype(bool)
    cpu.inflate_map((np.median(b["keys"][full], axis=0) + 0.5) * cfg.subbox_d_xyz * cfg.subbox_n)  # (around the obstacles)
    b = cpu.export_blocks()
    assert ((b["infl"] == ord("o")) & (b["occ"] != ord("o"))).sum() > 100
    if released:
        assert b["collapsed"].any()
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    rng = np.random.default_rng(11)
    lo, hi = b["keys"].min(0) * d * n - 1.0, (b["keys"].max(0) + 1) * d * n + 1.0
    parts = [rw.uniform_rays(rng, lo, hi, N_RANDOM, short=1.5), rw.special_rays(rng, lo, hi, d, count=250),
             rw.uniform_rays(rng, lo + 500.0, hi + 500.0, 60),  # absent space only
             rw.weird_rays(d)]
    p0, p1 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    classes = rw.block_classes(b, n)
    # the classes the walk reads are the oracle's point queries at the voxel centres (on a sample of voxels around the map)
    vox = rng.integers(np.floor(lo / d).astype(int), np.ceil(hi / d).astype(int), size=(20000, 3))
    qc = rw.query_classes(cpu.getOccupancy, cpu.getInflateOccupancy, cfg)(vox)
    assert np.array_equal(classes(vox), qc) and len(np.unique(qc)) >= 4
    exp, ties = rw.cast_all(p0, p1, d, classes)
    rw.non_vacuous(exp, ties, N_RANDOM)
    assert (exp[rw.OCC]["status"] == -1).sum() >= 8  # (the invalid rays)
    got = run_driver(exe, tmp_path / "rays.bin", cfg, b, p0, p1)
    for f in rw.FLAG_SETS:
        rw.assert_equal(got[f], exp[f], f"{name} flags={f}")
