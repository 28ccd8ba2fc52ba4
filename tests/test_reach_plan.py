"""mlm_export_reach on the CPU: its planner, its per-voxel rules under the device's tile schedule, and its interface.

* mlm_reach_plan (mlmapping_amd/csrc/mlm_host.h) built with g++ -fsanitize=address,undefined: the tile grid covers the box exactly
  (boxes that are no multiple of the tile, one voxel thick, the largest box the entry point admits), the scratch bytes match the
  formula restated here, refused arguments are refused.
* the rules of mlmapping_amd/csrc/mlm_reach.h (relaxation, face marking, parent: the code the kernels run) driven tile by tile with
  the dirty-array schedule of the host loop, sequentially, on masks generated here: every steps and parent value and the three
  pinned summary counters equal the breadth-first reference (tests/reach_ref.py), for several tile geometries; the schedule
  stops by itself below the plan's cap.
* the knobs' ranges, the binding's methods and constants."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import reach_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
HALO_VOXELS, GROUP_MAX, CTRL_BYTES = 15360, 256, 2048  # (mlm_host.h kReachHaloVoxels, kReachGroupMax, kReachCtrlBytes)


def pack(t):
    return t[0] | t[1] << 8 | t[2] << 16


DEFAULT_TILE = (32, 8, 8)
TILES = [DEFAULT_TILE, (1, 5, 3), (4, 4, 4), (7, 1, 2), (64, 2, 1)]  # (a single voxel wide on x, and on y)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("rp")
    exe = d / "reach_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "reach_driver.cpp"), "-o", str(exe)])

    def plan(*cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(exe), "plan", *args], check=True, capture_output=True, text=True).stdout
        return np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)

    def run(blocked, seeds, tile, max_steps=2 ** 31 - 1):
        dz, dy, dx = blocked.shape
        s = np.asarray(seeds, dtype=np.int32).reshape(-1, 3)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([dx, dy, dz, pack(tile), max_steps, len(s)], dtype=np.int64).tobytes())
            f.write(s.tobytes())
            f.write(np.ascontiguousarray(blocked, dtype=np.uint8).tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:48], dtype=np.int64)
        n = dx * dy * dz
        return {"summary": head[:3], "sweeps": int(head[3]), "cap": int(head[4]), "tiles": int(head[5]),
                "steps": np.frombuffer(raw[48:48 + 4 * n], dtype=np.int32).reshape(dz, dy, dx),
                "parent": np.frombuffer(raw[48 + 4 * n:], dtype=np.uint8).reshape(dz, dy, dx)}

    return plan, run


def up(v):
    return (v + 255) // 256 * 256


# ---- the planner --------------------------------------------------------------------------------------------------------------
def test_plan_grid_and_scratch(driver):
    plan, _ = driver
    boxes = [(1, 1, 1), (33, 9, 9), (32, 8, 8), (31, 7, 1), (1, 200, 3), (93, 73, 63), (512, 512, 64), (2 ** 31 - 1, 1, 1), (1, 1, 2 ** 31 - 1),
             (65536, 32767, 1), (1290, 1290, 1290)]
    cases = [(*D, pack(T), ns, ms) for D in boxes for T in TILES for ns, ms in ((1, 2 ** 31 - 1), (1000, 17))]
    rows = plan(*cases)
    assert len(rows) == len(cases)
    for r, c in zip(rows, cases):
        D, tile, ns, ms = np.array(c[:3]), c[3], c[4], c[5]
        assert tuple(r[:6]) == tuple(c) and r[6] == 1
        T, n, tiles, vox = r[7:10], r[10:13], r[13], r[14]
        assert tuple(T) == (tile & 255, tile >> 8 & 255, tile >> 16)
        # the grid covers the box exactly: the last tile per axis starts inside the box and ends at or beyond its edge
        assert ((n - 1) * T < D).all() and (n * T >= D).all()
        assert tiles == int(n[0]) * int(n[1]) * int(n[2]) and vox == int(D[0]) * int(D[1]) * int(D[2])
        fb, mb, db, sb = r[15:19]
        assert (fb, mb, db, sb) == (up(4 * vox), up(vox), up(tiles), up(12 * ns))
        assert tuple(r[19:23]) == (fb, fb + mb, fb + mb + 2 * db, fb + mb + 2 * db + CTRL_BYTES)
        assert r[23] == fb + mb + 2 * db + CTRL_BYTES + sb
        assert r[24] == min(ms, vox - 1) + 2
        assert (T[0] + 2) * (T[1] + 2) * (T[2] + 2) <= HALO_VOXELS


def test_plan_tiles_cover_each_voxel_once(driver):
    plan, _ = driver
    for D in [(33, 9, 9), (5, 1, 7), (70, 3, 2)]:
        for T in TILES:
            r = plan((*D, pack(T), 1, 5))[0]
            n = r[10:13]
            cover = np.zeros(D[::-1], dtype=np.int32)
            for t2 in range(n[2]):
                for t1 in range(n[1]):
                    for t0 in range(n[0]):
                        cover[t2 * T[2]:(t2 + 1) * T[2], t1 * T[1]:(t1 + 1) * T[1], t0 * T[0]:(t0 + 1) * T[0]] += 1
            assert (cover == 1).all(), (D, T)


def test_plan_refusals(driver):
    plan, _ = driver
    bad_tiles = [0, pack((0, 8, 8)), pack((8, 0, 8)), pack((8, 8, 0)), pack((65, 1, 1)), pack((64, 64, 64)), pack((30, 30, 30)), 1 << 24, -1]
    cases = [(4, 4, 4, t, 1, 5) for t in bad_tiles]
    cases += [(0, 4, 4, pack(DEFAULT_TILE), 1, 5), (4, -1, 4, pack(DEFAULT_TILE), 1, 5), (4, 4, 4, pack(DEFAULT_TILE), 0, 5),
              (4, 4, 4, pack(DEFAULT_TILE), 1, 0), (4, 4, 4, pack(DEFAULT_TILE), 1, -3)]
    rows = plan(*cases)
    assert (rows[:, 6] == 0).all()
    ok = plan((4, 4, 4, pack((22, 22, 22)), 1, 1), (4, 4, 4, pack((64, 13, 13)), 1, 1))  # (24^3 = 13 824, 66 * 15 * 15 = 14 850)
    assert (ok[:, 6] == 1).all()


# ---- the rules under the tile schedule ----------------------------------------------------------------------------------------
def compare(run, blocked, seeds, max_steps=None, tiles=TILES, what=""):
    exp = ref.reach(~blocked, seeds, max_steps)
    for T in tiles:
        got = run(blocked, seeds, T, 2 ** 31 - 1 if max_steps is None else max_steps)
        assert np.array_equal(got["steps"], exp["steps"]), (what, T)
        assert np.array_equal(got["parent"], exp["parent"]), (what, T)
        assert np.array_equal(got["summary"], exp["summary"]), (what, T)
        assert 1 <= got["sweeps"] <= got["cap"], (what, T, got["sweeps"], got["cap"])
    return exp


def test_open_box_is_manhattan(driver):
    _, run = driver
    blocked = np.zeros((9, 20, 41), dtype=bool)
    seed = (17, 3, 5)
    exp = compare(run, blocked, [seed], what="open")
    z, y, x = np.indices(blocked.shape)
    assert np.array_equal(exp["steps"], abs(x - seed[0]) + abs(y - seed[1]) + abs(z - seed[2]))
    assert exp["parent"][seed[2], seed[1], seed[0]] == ref.SEED
    assert ref.walk(exp["parent"], (40, 19, 8))[-1] == seed


def test_serpentines(driver):
    """shortest paths many times the box edge: every tile is entered again and again"""
    _, run = driver
    slab = ref.serpentine_slab(64, 64)
    exp = compare(run, slab, [(0, 0, 0)], what="slab")
    assert exp["summary"][2] >= 20 * 64 and exp["summary"][0] == exp["summary"][1]
    maze = ref.serpentine_3d(16)
    exp = compare(run, maze, [(0, 0, 0)], tiles=[(4, 4, 4), (1, 5, 3), DEFAULT_TILE], what="maze")
    assert exp["summary"][2] >= 20 * 16 and exp["summary"][0] == exp["summary"][1]
    assert len(ref.walk(exp["parent"], np.unravel_index(exp["steps"].argmax(), maze.shape)[::-1])) == exp["summary"][2] + 1


@pytest.mark.parametrize("density", [0.3, 0.45, 0.6])
def test_random_masks(driver, density):
    _, run = driver
    rng = np.random.default_rng(int(density * 100))
    for shape in [(7, 19, 37), (1, 40, 33), (12, 1, 50)]:
        blocked = rng.random(shape) < density
        free = np.argwhere(~blocked)[:, ::-1]
        one = free[rng.integers(len(free))]
        compare(run, blocked, [one], what=f"one seed {shape}")
        several = free[rng.integers(len(free), size=5)]
        on_obstacle = np.argwhere(blocked)[:3, ::-1]
        outside = np.array([[-1, 0, 0], [shape[2], 0, 0], [0, shape[1], 0], [0, 0, -5], [2 ** 31 - 1, 0, 0]])
        exp = compare(run, blocked, np.concatenate([several, on_obstacle, outside, several[:2]]), what=f"several {shape}")
        assert (exp["parent"] == ref.SEED).sum() == len(np.unique(several, axis=0))
        none = compare(run, blocked, np.concatenate([on_obstacle, outside]), what=f"no effective seed {shape}")
        assert none["summary"][1] == 0 and none["summary"][2] == -1 and (none["parent"] == 255).all()


def test_max_steps_truncation(driver):
    _, run = driver
    rng = np.random.default_rng(5)
    blocked = rng.random((6, 25, 30)) < 0.3
    seed = np.argwhere(~blocked)[0, ::-1]
    full = ref.reach(~blocked, [seed])
    assert full["summary"][2] > 12
    for ms in (1, 4, 12):
        exp = compare(run, blocked, [seed], max_steps=ms, what=f"max_steps {ms}")
        assert np.array_equal(exp["steps"], np.where(full["steps"] <= ms, full["steps"], -1))
        assert exp["summary"][2] == ms


def test_reference_forms_agree():
    """the breadth-first reference against scipy's connected components (where scipy imports) and its own blocked mask against
    the definition taken literally"""
    rng = np.random.default_rng(11)
    blocked = rng.random((8, 21, 17)) < 0.55
    seed = np.argwhere(~blocked)[7, ::-1]
    r = ref.reach(~blocked, [seed])
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        lab, _ = ndimage.label(~blocked)  # (6-connectivity is scipy's default structure)
        assert np.array_equal(r["steps"] >= 0, lab == lab[seed[2], seed[1], seed[0]])
    for rad in (0, 1, 2, 3):
        g = rad + 1
        obs = rng.random((6 + 2 * g, 9 + 2 * g, 11 + 2 * g)) < 0.02  # the box grown by rad + 1; the map holds nothing else
        b = ref.blocked(obs, rad)
        assert b.shape == (6, 9, 11)
        v = np.argwhere(np.ones(b.shape, dtype=bool)) + g
        d2 = ((v[:, None, :] - np.argwhere(obs)[None, :, :]) ** 2).sum(-1).min(1)
        assert np.array_equal(b.ravel(), d2 <= rad * rad), rad
        assert b.any() and not b.all()


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_knob_ranges():
    from mlmapping_amd.mlmap import load_library

    L = load_library()
    try:
        for T in TILES + [(1, 1, 1), (22, 22, 22), (64, 13, 13)]:
            assert L.mlm_debug_set(b"reach_tile", pack(T)) == 0, T
        for v in (0, -1, pack((0, 8, 8)), pack((65, 1, 1)), pack((64, 64, 64)), pack((23, 23, 23)) + (1 << 24), 1 << 24, 1 << 40):
            assert L.mlm_debug_set(b"reach_tile", v) == -1, v
        for v in (1, 8, 64, GROUP_MAX):
            assert L.mlm_debug_set(b"reach_group", v) == 0, v
        for v in (0, -1, GROUP_MAX + 1, 1 << 40):
            assert L.mlm_debug_set(b"reach_group", v) == -1, v
    finally:
        L.mlm_debug_reset()


def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_REACH_OCC, mlmap.MLM_REACH_INFL, mlmap.MLM_REACH_UNKNOWN, mlmap.MLM_REACH_NONE, mlmap.MLM_REACH_SEED) == (1, 2, 4, -1, 6)
    assert callable(mlmap.MLMap.export_reach) and callable(mlmap.MLMap.export_reach_dev)
    assert "mlm_export_reach" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_reach")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("OCC", "1"), ("INFL", "2"), ("UNKNOWN", "4"), ("NONE", r"\(-1\)"), ("SEED", "6")):
        assert re.search(rf"#define MLM_REACH_{name} {v}(\s|$)", hdr), name
    assert (ref.NONE, ref.SEED) == (mlmap.MLM_REACH_NONE, mlmap.MLM_REACH_SEED)
