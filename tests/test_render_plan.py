"""mlm_render_depth on the host: the pinhole arithmetic of mlmapping_amd/csrc/mlm_render.h (what the kernel k_render runs too) in front
of the walk of mlm_raywalk.h, built for the CPU with -fsanitize=address,undefined and held to the contract's arithmetic in numpy
float64 (tests/render_ref.py) and the walk in plain Python integers (tests/raywalk_ref.py) over the oracle's voxel classes: every
integer exactly, the end points and t by their 64 bits, the depth exactly, every flag set, on a map with released and absent blocks."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from mlmapping_amd.mlmap import compose_T_ws
from tests import raywalk_ref as rw
from tests import render_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = S1.with_(use_exploration_frontiers=True, subbox_n=5)
D, N = CFG.subbox_d_xyz, CFG.subbox_n
SHIFT = np.array([-8.0, -7.5, 0.0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("render") / "render_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "render_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def world():
    """the block dump of a frontier-mode map in negative x, y (released blocks, inflation), its classes and the poses that built it"""
    from oracle.binding import OracleMap

    cpu = OracleMap(CFG)
    poses = []
    for img, (q, t) in syn.stream(CFG, "room_jitter", "smooth", 4):
        cpu.update_depth(img, q, np.array(t) + SHIFT)
        poses.append((q, np.array(t) + SHIFT))
    b = cpu.export_blocks()
    full = (b["occ"] == ord("o")).any(axis=1) & ~b["collapsed"].astype(bool)
    cpu.inflate_map((np.median(b["keys"][full], axis=0) + 0.5) * D * N)
    b = cpu.export_blocks()
    assert b["collapsed"].any() and ((b["infl"] == ord("o")) & (b["occ"] != ord("o"))).sum() > 100
    classes = rw.block_classes(b, N)
    rng = np.random.default_rng(3)  # the classes the walk reads are the oracle's point queries at the voxel centres
    vox = rng.integers(b["keys"].min(0) * N - 10, (b["keys"].max(0) + 1) * N + 10, size=(20000, 3))
    assert np.array_equal(classes(vox), rw.query_classes(cpu.getOccupancy, cpu.getInflateOccupancy, CFG)(vox))
    return b, classes, poses


def run_driver(exe, path, d, b, cases, depth_cases=(), flag_sets=rw.FLAG_SETS):
    """cases: (T_ws (12,), K (4,), max_depth_mm, width, height); depth_cases: (status, max_depth_mm, t).  Returns per case
    {flags: outputs}, p0, p1 — and the depths of depth_cases"""
    blob = struct.pack("<d5i", d, N, b["keys"].shape[0], len(flag_sets), len(cases), len(depth_cases))
    blob += np.array(flag_sets, dtype=np.int32).tobytes()
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    for T, K, mm, w, h in cases:
        blob += np.asarray(T, dtype=np.float64).reshape(12).tobytes() + np.asarray(K, dtype=np.float64).reshape(4).tobytes() + struct.pack("<3i", mm, w, h)
    for st, mm, t in depth_cases:
        blob += struct.pack("<2id", st, mm, t)
    path.write_bytes(blob)
    rows = [ln.split() for ln in subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    out, at = [], 0
    for T, K, mm, w, h in cases:
        per = {}
        for f in flag_sets:
            r = rows[at:at + w * h]
            at += w * h
            per[f] = {"status": np.array([int(x[0]) for x in r], dtype=np.int8), "voxel": np.array([[int(v) for v in x[1:4]] for x in r], dtype=np.int32).reshape(-1, 3),
                      "t": np.array([float.fromhex(x[4]) for x in r], dtype=np.float64), "n_steps": np.array([int(x[5]) for x in r], dtype=np.int32),
                      "n_unknown": np.array([int(x[6]) for x in r], dtype=np.int32), "depth": np.array([int(x[7]) for x in r], dtype=np.uint16),
                      "p0": np.array([[float.fromhex(v) for v in x[8:11]] for x in r], dtype=np.float64).reshape(-1, 3),
                      "p1": np.array([[float.fromhex(v) for v in x[11:14]] for x in r], dtype=np.float64).reshape(-1, 3)}
        out.append(per)
    depths = [int(x[0]) for x in rows[at:]]
    assert len(depths) == len(depth_cases)
    return out, depths


def same_doubles(a, b):
    """by their 64 bits; a NaN equals a NaN (printf does not carry its payload)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def check_case(got, case, d, classes, what):
    T, K, mm, w, h = case
    exp, p0, p1, ties = rr.render_all(np.asarray(T).reshape(1, 12), w, h, K, mm, d, classes)
    for f in rw.FLAG_SETS:
        assert same_doubles(got[f]["p0"], p0) and same_doubles(got[f]["p1"], p1), (what, f)
        rw.assert_equal(got[f], exp[f], f"{what} flags={f}")
        assert got[f]["depth"].dtype == exp[f]["depth"].dtype and np.array_equal(got[f]["depth"], exp[f]["depth"]), (what, f)
        assert np.array_equal((got[f]["depth"] == 0), (exp[f]["status"] != 1)), (what, f)  # depth == 0 iff nothing stopped the ray
    return exp, ties


def test_images_equal_the_numpy_segments_and_the_python_walk(exe, world, tmp_path):
    b, classes, poses = world
    K = (30.0, 28.0, 8.3, 5.6)  # a 17 x 11 image with a 30-degree half angle
    W, H = 17, 11
    T_cam = compose_T_ws(np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]), CFG.T_B_S)  # the (tilted, jittering) poses of the frames
    eye = np.concatenate([np.eye(3).reshape(9), poses[0][1]])
    # a camera inside an occupied voxel of a block that is not released
    blk = np.flatnonzero((b["occ"] == ord("o")).any(axis=1) & ~b["collapsed"].astype(bool))[0]
    cid = int(np.flatnonzero(b["occ"][blk] == ord("o"))[0])
    inside_vox = b["keys"][blk].astype(np.int64) * N + np.array([cid % N, (cid // N) % N, cid // (N * N)])
    inside = np.concatenate([T_cam[1, :9], (inside_vox + 0.5) * D])
    outside = np.concatenate([T_cam[0, :9], poses[0][1] + 500.0])  # outside every block: all UNKNOWN
    nan_pose, inf_pose = T_cam[0].copy(), T_cam[2].copy()
    nan_pose[4] = np.nan
    inf_pose[10] = np.inf
    # rays exactly along voxel faces: cx, cy and o on the lattice, the rotation the identity — the column u = cx runs in the plane
    # x = o.x, the row v = cy in the plane y = o.y, the pixel (cx, cy) along an edge
    lat = np.concatenate([np.eye(3).reshape(9), np.round((poses[0][1] - [0, 0, 1.0]) / D) * D])
    K_lat = (30.0, 28.0, 8.0, 5.0)
    K_tall = (30.0, 10.0, 8.3, 5.6)  # (tall enough to see floor and ceiling in front of the far wall, which a 3.9 m ray does not reach)
    cases = [(T_cam[0], K_tall, 3900, W, H), (T_cam[3], K, 8000, W, H), (eye, K, 4000, W, H), (inside, K, 4000, 5, 4), (outside, K, 4000, 5, 4),
             (nan_pose, K, 4000, 5, 4), (inf_pose, K, 4000, 5, 4), (T_cam[1], K, 1, 5, 4), (T_cam[2], K, 65535, 9, 7), (lat, K_lat, 4000, W, H),
             (T_cam[0], (30.0, 28.0, -2.5, 400.25), 3000, 6, 3)]  # (a principal point outside the image)
    names = ["pose 0", "pose 3 at 8 m", "identity", "inside an obstacle", "outside every block", "NaN", "Inf", "1 mm", "65.535 m", "on the lattice",
             "off-centre"]
    got, _ = run_driver(exe, tmp_path / "render.bin", D, b, cases)
    exps = {}
    for name, g, case in zip(names, got, cases):
        exps[name] = check_case(g, case, D, classes, name)
    occ = lambda name: exps[name][0][rw.OCC]
    # what the cases are there for
    st = np.concatenate([occ("pose 0")["status"], occ("pose 3 at 8 m")["status"]])
    assert (st == 1).sum() >= len(st) // 10 and (st == 0).sum() >= len(st) // 10, ((st == 1).sum(), (st == 0).sum())
    assert (exps["65.535 m"][0][0]["n_unknown"] > 0).any() and len(np.unique(occ("pose 3 at 8 m")["depth"])) > 10
    assert np.all(occ("inside an obstacle")["status"] == 1) and np.all(occ("inside an obstacle")["depth"] == 1) and np.all(occ("inside an obstacle")["t"] == 0.0)
    assert np.all(occ("outside every block")["status"] == 0) and np.all(occ("outside every block")["n_unknown"] == occ("outside every block")["n_steps"])
    assert np.all(exps["outside every block"][0][rw.UNKNOWN]["depth"] == 1)
    for name in ("NaN", "Inf"):
        for f in rw.FLAG_SETS:
            assert np.all(exps[name][0][f]["status"] == -1) and np.all(exps[name][0][f]["depth"] == 0), (name, f)
    assert np.all(occ("1 mm")["status"] >= 0) and np.all(occ("1 mm")["n_steps"] <= 2)
    assert np.all(occ("65.535 m")["status"] >= 0) and exps["65.535 m"][0][0]["n_steps"].max() > 600
    assert (exps["on the lattice"][1] > 0).sum() >= W + H - 1  # (tie steps: the column, the row)
    # the depth is the z-depth: straight ahead of the tilted camera and in the corner of the image it is the same plane
    assert occ("pose 3 at 8 m")["depth"].max() <= 8000


def test_a_voxel_so_small_that_the_depth_range_exceeds_the_lattice(exe, world, tmp_path):
    """subbox_d_xyz = 1 mm: 65.535 m are 65 535 voxels along the optical axis, more than the 32 768 a ray may span — every pixel is
    invalid; at 32.7 m the same camera is valid"""
    b, classes, poses = world
    d = 0.001
    T = np.concatenate([np.eye(3).reshape(9), [0.0123, -0.0456, 0.0789]])
    K = (30.0, 28.0, 2.2, 1.6)
    cases = [(T, K, 65535, 5, 4), (T, K, 32700, 2, 1)]
    got, _ = run_driver(exe, tmp_path / "small.bin", d, b, cases, flag_sets=(0, rw.UNKNOWN))
    for f in (0, rw.UNKNOWN):
        assert np.all(got[0][f]["status"] == -1) and np.all(got[0][f]["depth"] == 0) and np.all(got[0][f]["n_steps"] == 0)
    for k, case in enumerate(cases):
        exp, p0, p1, _ = rr.render_all(np.asarray(case[0]).reshape(1, 12), case[3], case[4], case[1], case[2], d, classes, (0, rw.UNKNOWN))
        for f in (0, rw.UNKNOWN):
            assert same_doubles(got[k][f]["p1"], p1)
            rw.assert_equal(got[k][f], exp[f], f"1 mm voxels case {k} flags={f}")
            assert np.array_equal(got[k][f]["depth"], exp[f]["depth"])
    assert np.all(got[1][0]["status"] == 0) and got[1][0]["n_steps"].min() > 32700


def test_depth_rounding(exe, world, tmp_path):
    """z + 0.5 an exact integer rounds up (floor(z + 0.5)); a stop never reports 0; no stop and invalid report 0; 65535 is the cap"""
    b, _, _ = world
    hand = [((1, 1001, 0.5), 501), ((1, 2002, 0.25), 501), ((1, 3, 0.5), 2), ((1, 2, 0.25), 1), ((1, 4000, 0.0), 1), ((1, 1, 0.25), 1), ((1, 65535, 1.0), 65535),
            ((1, 65535, 0.999999), 65535), ((0, 4000, 1.0), 0), ((-1, 4000, 0.0), 0), ((1, 4000, 0.6251), 2500), ((1, 4000, 0.625125), 2501)]
    for (st, mm, t), want in hand[:4]:
        assert (t * mm + 0.5) == float(int(t * mm + 0.5))  # (the halves are exact)
    rng = np.random.default_rng(8)
    m = rng.integers(0, 1 << 25, size=400)
    ad = np.maximum(m, rng.integers(1, 1 << 25, size=400))
    rand = [(1, int(mm), float(a) / float(c)) for mm, a, c in zip(rng.integers(1, 65536, size=400), m, ad)]  # t = m / |D| as the walk forms it
    cases = [c for c, _ in hand] + rand
    _, depths = run_driver(exe, tmp_path / "depth.bin", D, b, [], depth_cases=cases)
    assert depths[:len(hand)] == [w for _, w in hand]
    exp = [int(rr.depth_mm(st, t, mm)) for st, mm, t in cases]
    assert depths == exp
