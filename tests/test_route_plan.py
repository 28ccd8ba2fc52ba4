"""mlm_export_route on the CPU: its planner, its per-voxel rules under the device's tile schedule, its reference and its interface.

* mlm_route_plan (mlmapping_amd/csrc/mlm_host.h) built with g++ -fsanitize=address,undefined: the tile grid covers the box exactly,
  the scratch and LDS bytes match the formulas restated here, refused arguments are refused, the cap is voxels + 1.
* the rules of mlmapping_amd/csrc/mlm_route.h (ring classes, permitted moves, relaxation, dirty tiles, parent: the code the kernels
  run) driven tile by tile with the dirty-array schedule of the host loop, sequentially, on masks generated here: every cost and
  parent value and the three pinned summary counters equal the numpy reference (tests/route_ref.py), for the three
  connectivities, several tile geometries, move costs and penalties; the schedule stops by itself below the plan's cap.
* the reference's two forms against each other, the 6-connected unit-cost field against tests/reach_ref.py, corner cutting,
  max_cost, the knobs' ranges, the binding's methods and constants."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import reach_ref
from tests import route_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
HALO_VOXELS, GROUP_MAX, CTRL_BYTES = 15360, 256, 2048  # (mlm_host.h kReachHaloVoxels, kReachGroupMax, kReachCtrlBytes)


def pack(t):
    return t[0] | t[1] << 8 | t[2] << 16


DEFAULT_TILE = (32, 8, 8)
TILES = [DEFAULT_TILE, (1, 5, 3), (4, 4, 4), (7, 1, 2), (64, 2, 1)]
SHAPES = [(7, 19, 37), (1, 40, 33), (12, 1, 50)]
COSTS = [(10, 14, 17), (3, 3, 3)]
PENALTIES = [(), (40, 15, 5)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("rt")
    exe = d / "route_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "route_driver.cpp"), "-o", str(exe)])

    def plan(*cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(exe), "plan", *args], check=True, capture_output=True, text=True).stdout
        return np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)

    def run(d_out, seeds, tile, connectivity, move_cost, penalty, clearance=0, max_cost=2 ** 31 - 1):
        dz, dy, dx = d_out.shape
        s = np.asarray(seeds, dtype=np.int32).reshape(-1, 3)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([dx, dy, dz, pack(tile), max_cost, len(s), connectivity, *move_cost, clearance, len(penalty)], dtype=np.int64).tobytes())
            f.write(np.asarray(penalty, dtype=np.int32).tobytes())
            f.write(s.tobytes())
            f.write(np.ascontiguousarray(d_out, dtype=np.uint16).tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:48], dtype=np.int64)
        n = dx * dy * dz
        return {"summary": head[:3], "sweeps": int(head[3]), "cap": int(head[4]), "tiles": int(head[5]),
                "cost": np.frombuffer(raw[48:48 + 4 * n], dtype=np.int32).reshape(dz, dy, dx),
                "parent": np.frombuffer(raw[48 + 4 * n:48 + 5 * n], dtype=np.uint8).reshape(dz, dy, dx),
                "cls": np.frombuffer(raw[48 + 5 * n:], dtype=np.uint8).reshape(dz, dy, dx)}

    return plan, run


def up(v):
    return (v + 255) // 256 * 256


# ---- the planner --------------------------------------------------------------------------------------------------------------
def test_plan_grid_scratch_and_cap(driver):
    plan, _ = driver
    boxes = [(1, 1, 1), (33, 9, 9), (32, 8, 8), (31, 7, 1), (1, 200, 3), (93, 73, 63), (512, 512, 64), (2 ** 31 - 1, 1, 1), (1, 1, 2 ** 31 - 1),
             (65536, 32767, 1), (1290, 1290, 1290)]
    cases = [(*D, pack(T), ns) for D in boxes for T in TILES + [(22, 22, 22), (64, 13, 13)] for ns in (1, 1000)]
    rows = plan(*cases)
    assert len(rows) == len(cases)
    for r, c in zip(rows, cases):
        D, tile, ns = np.array(c[:3]), c[3], c[4]
        assert tuple(r[:5]) == tuple(c) and r[5] == 1
        T, n, tiles, vox = r[6:9], r[9:12], r[12], r[13]
        assert tuple(T) == (tile & 255, tile >> 8 & 255, tile >> 16)
        # the grid covers the box exactly: the last tile per axis starts inside the box and ends at or beyond its edge
        assert ((n - 1) * T < D).all() and (n * T >= D).all()
        assert tiles == int(n[0]) * int(n[1]) * int(n[2]) and vox == int(D[0]) * int(D[1]) * int(D[2])
        fb, cb, db, sb = r[14:18]
        assert (fb, cb, db, sb) == (up(4 * vox), up(vox), up(tiles), up(12 * ns))  # 4 B of cost and a class byte per voxel, a dirty byte per tile
        assert tuple(r[18:22]) == (fb, fb + cb, fb + cb + 2 * db, fb + cb + 2 * db + CTRL_BYTES)
        assert r[22] == fb + cb + 2 * db + CTRL_BYTES + sb
        halo = (T[0] + 2) * (T[1] + 2) * (T[2] + 2)
        assert halo <= HALO_VOXELS and r[23] == 4 * halo + 2 * T[0] * T[1] * T[2] and r[23] < 160 * 1024
        assert r[24] == vox + 1
    assert plan((93, 73, 63, pack(DEFAULT_TILE), 1))[0][23] == 17696


def test_plan_tiles_cover_each_voxel_once(driver):
    plan, _ = driver
    for D in [(33, 9, 9), (5, 1, 7), (70, 3, 2)]:
        for T in TILES:
            n = plan((*D, pack(T), 1))[0][9:12]
            cover = np.zeros(D[::-1], dtype=np.int32)
            for t2 in range(n[2]):
                for t1 in range(n[1]):
                    for t0 in range(n[0]):
                        cover[t2 * T[2]:(t2 + 1) * T[2], t1 * T[1]:(t1 + 1) * T[1], t0 * T[0]:(t0 + 1) * T[0]] += 1
            assert (cover == 1).all(), (D, T)


def test_plan_refusals(driver):
    plan, _ = driver
    bad_tiles = [0, pack((0, 8, 8)), pack((8, 0, 8)), pack((8, 8, 0)), pack((65, 1, 1)), pack((64, 64, 64)), pack((30, 30, 30)), 1 << 24, -1]
    cases = [(4, 4, 4, t, 1) for t in bad_tiles]
    cases += [(0, 4, 4, pack(DEFAULT_TILE), 1), (4, -1, 4, pack(DEFAULT_TILE), 1), (4, 4, 4, pack(DEFAULT_TILE), 0), (4, 4, 4, pack(DEFAULT_TILE), -2)]
    assert (plan(*cases)[:, 5] == 0).all()
    assert (plan((4, 4, 4, pack((22, 22, 22)), 1), (4, 4, 4, pack((64, 13, 13)), 1))[:, 5] == 1).all()


# ---- the reference ------------------------------------------------------------------------------------------------------------
def grown_obstacles(rng, shape, density, g):
    """a random obstacle mask of the box grown by g voxels per side (obstacles beyond the box count for the rings)"""
    return rng.random(tuple(n + 2 * g for n in shape)) < density


def d_out_of(obs, g):
    """what the ESDF passes hand to the classification: min(g^2, squared distance to the nearest obstacle) on the box"""
    return reach_ref.edt_separable(obs, g)[g:-g, g:-g, g:-g]


def test_offsets_and_intermediates():
    assert ref.OFFSETS[:6] == [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    assert (ref.OFFSETS[6], ref.OFFSETS[10], ref.OFFSETS[17], ref.OFFSETS[18], ref.OFFSETS[25]) == ((0, -1, -1), (-1, -1, 0), (0, 1, 1), (-1, -1, -1), (1, 1, 1))
    assert len(set(ref.OFFSETS)) == 26 and (0, 0, 0) not in ref.OFFSETS
    assert [np.count_nonzero(o) for o in ref.OFFSETS] == [1] * 6 + [2] * 12 + [3] * 8
    assert sorted(ref.intermediates((1, -1, 0))) == [(0, -1, 0), (1, 0, 0)]
    assert sorted(ref.intermediates((1, -1, 1))) == sorted([(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, -1, 0), (1, 0, 1), (0, -1, 1)])
    assert ref.intermediates((0, 0, -1)) == []


def test_reference_forms_agree():
    """the label-correcting reference against the heapq Dijkstra, and the ring classes against the definition taken literally"""
    rng = np.random.default_rng(11)
    for conn, costs, pen, r in ((26, (10, 14, 17), (40, 15, 5), 0), (18, (3, 3, 3), (), 0), (6, (1, 1, 1), (7,), 1), (26, (5, 9, 6), (2, 0, 9), 1)):
        g = r + len(pen) + 1
        obs = grown_obstacles(rng, (8, 21, 17), 0.3 if r == 0 and not pen else 0.01, g)  # (sparse where every ring must occur)
        cls = ref.classes(obs, r, len(pen))
        assert cls.shape == (8, 21, 17)
        # the definition: blocked iff some obstacle within r^2; ring k: the smallest k with D <= (r + 1 + k)^2
        v = np.argwhere(np.ones(cls.shape, dtype=bool)) + g
        d2 = ((v[:, None, :] - np.argwhere(obs)[None, :, :]) ** 2).sum(-1).min(1).reshape(cls.shape)
        exp = np.full(cls.shape, len(pen), dtype=np.uint8)
        for k in range(len(pen) - 1, -1, -1):
            exp[d2 <= (r + 1 + k) ** 2] = k
        exp[d2 <= r * r] = ref.BLOCKED
        assert np.array_equal(cls, exp)
        assert all((cls == k).any() for k in list(range(len(pen) + 1)) + [ref.BLOCKED])
        free = np.argwhere(cls != ref.BLOCKED)[:, ::-1]
        seeds = free[rng.integers(len(free), size=2)]
        a = ref.route(cls, seeds, conn, costs, pen)
        assert np.array_equal(a["cost"], ref.dijkstra(cls, seeds, conn, costs, pen)), conn
        assert a["summary"][1] > 100
        far = np.unravel_index(a["cost"].argmax(), cls.shape)[::-1]
        path = ref.walk(a["parent"], far)  # the parents walk a path of exactly that cost
        total = sum(costs[np.count_nonzero(np.subtract(p, q)) - 1] + ref.pen_of(cls, pen)[p[2], p[1], p[0]] for p, q in zip(path[:-1], path[1:]))
        assert total == a["cost"][far[2], far[1], far[0]] and a["parent"][path[-1][2], path[-1][1], path[-1][0]] == ref.SEED
        cut = int(a["summary"][2]) // 2
        assert np.array_equal(ref.dijkstra(cls, seeds, conn, costs, pen, cut), np.where(a["cost"] <= cut, a["cost"], -1))


def test_unit_cost_6_is_reach():
    rng = np.random.default_rng(3)
    blocked = rng.random((8, 21, 17)) < 0.4
    seeds = np.argwhere(~blocked)[[5, 90], ::-1]
    cls = np.where(blocked, ref.BLOCKED, 0).astype(np.uint8)
    for ms in (None, 9):
        a, b = ref.route(cls, seeds, 6, (1, 1, 1), (), ms), reach_ref.reach(~blocked, seeds, ms)
        assert np.array_equal(a["cost"], b["steps"]) and np.array_equal(a["summary"], b["summary"])
        assert np.array_equal(a["parent"], np.where(b["parent"] == reach_ref.SEED, ref.SEED, b["parent"]))


# ---- the rules under the tile schedule ----------------------------------------------------------------------------------------
def compare(run, obs, g, seeds, conn, costs, pen, r=0, max_cost=None, tiles=TILES, what=""):
    """obs: the obstacle mask of the box grown by g = r + len(pen) + 1"""
    exp = ref.route(ref.classes(obs, r, len(pen)), seeds, conn, costs, pen, max_cost)
    for T in tiles:
        got = run(d_out_of(obs, g), seeds, T, conn, costs, pen, r, 2 ** 31 - 1 if max_cost is None else max_cost)
        assert np.array_equal(got["cls"], ref.classes(obs, r, len(pen))), (what, T)
        for k in ("cost", "parent", "summary"):
            assert np.array_equal(got[k], exp[k]), (what, T, k)
        assert 1 <= got["sweeps"] <= got["cap"], (what, T, got["sweeps"], got["cap"])
    return exp


@pytest.mark.parametrize("conn", [6, 18, 26])
@pytest.mark.parametrize("density", [0.3, 0.45])
def test_random_masks(driver, conn, density):
    _, run = driver
    rng = np.random.default_rng(int(density * 100) + conn)
    for shape in SHAPES:
        for costs in COSTS:
            for pen in PENALTIES:
                g = len(pen) + 1
                obs = grown_obstacles(rng, shape, density, g)
                blocked = obs[g:-g, g:-g, g:-g]
                free = np.argwhere(~blocked)[:, ::-1]
                several = free[rng.integers(len(free), size=4)]
                on_obstacle = np.argwhere(blocked)[:3, ::-1]
                outside = np.array([[-1, 0, 0], [shape[2], 0, 0], [0, shape[1], 0], [0, 0, -5], [2 ** 31 - 1, 0, 0]])
                exp = compare(run, obs, g, np.concatenate([several, on_obstacle, outside, several[:2]]), conn, costs, pen,
                              what=f"{shape} {costs} {pen}")
                assert (exp["parent"] == ref.SEED).sum() == len(np.unique(several, axis=0))
    none = compare(run, obs, g, np.concatenate([on_obstacle, outside]), conn, costs, pen, tiles=[DEFAULT_TILE, (4, 4, 4)], what="no effective seed")
    assert none["summary"][1] == 0 and none["summary"][2] == -1 and (none["parent"] == 255).all()


def test_open_box_closed_form_and_clearance(driver):
    """no obstacle: 10 a + 4 b + 3 c over the sorted absolute offsets; a clearance with rings around sparse obstacles"""
    _, run = driver
    shape, seed = (9, 20, 41), (17, 3, 5)
    exp = compare(run, np.zeros(tuple(n + 2 for n in shape), dtype=bool), 1, [seed], 26, (10, 14, 17), (), what="open")
    z, y, x = np.indices(shape)
    d = np.sort(np.stack([abs(x - seed[0]), abs(y - seed[1]), abs(z - seed[2])]), axis=0)
    assert np.array_equal(exp["cost"], 10 * d[2] + 4 * d[1] + 3 * d[0])
    assert ref.walk(exp["parent"], (40, 19, 8))[-1] == seed
    rng = np.random.default_rng(8)
    for r, pen, conn in ((1, (30, 10), 26), (2, (9,), 18), (3, (), 6)):
        g = r + len(pen) + 1
        obs = grown_obstacles(rng, (6, 25, 30), 0.01, g)
        cls = ref.classes(obs, r, len(pen))
        free = np.argwhere(cls != ref.BLOCKED)[:, ::-1]
        exp = compare(run, obs, g, free[[0, len(free) // 2]], conn, (10, 14, 17), pen, r=r, tiles=[DEFAULT_TILE, (4, 4, 4), (7, 1, 2)], what=f"r={r}")
        assert exp["summary"][1] > 500 and all((cls == k).any() for k in range(len(pen) + 1))


def corner_pair(nx=9, ny=8, x=4, y=3):
    """a slab one voxel thick with obstacles at (x, y) and (x + 1, y + 1)"""
    b = np.zeros((1, ny, nx), dtype=bool)
    b[0, y, x] = b[0, y + 1, x + 1] = True
    return b


def diagonal_wall(n=12):
    """a slab one voxel thick with the obstacles (i, i): every diagonal move across the wall brushes two of them"""
    b = np.zeros((1, n, n), dtype=bool)
    b[0, np.arange(n), np.arange(n)] = True
    return b


def grow(blocked):
    return np.pad(blocked, 1, constant_values=False)


def test_corner_cutting(driver):
    _, run = driver
    pair = corner_pair()
    for conn in (18, 26):
        exp = compare(run, grow(pair), 1, [(5, 3, 0)], conn, (10, 14, 17), (), what="pair")
        assert exp["cost"][0, 4, 4] > 2 * 14  # (5, 3) -> (4, 4): not the diagonal between the two obstacles, but round one of them
        assert exp["cost"][0, 2, 6] == 14     # a free diagonal next to it
    wall = diagonal_wall()
    for conn in (6, 18, 26):
        exp = compare(run, grow(wall), 1, [(7, 2, 0)], conn, (10, 14, 17), (), what="wall")
        y, x = np.indices(wall.shape[1:])
        assert ((exp["cost"][0] >= 0) == (x > y)).all()


def test_max_cost_truncation(driver):
    _, run = driver
    rng = np.random.default_rng(5)
    obs = grown_obstacles(rng, (6, 25, 30), 0.3, 3)
    cls = ref.classes(obs, 0, 2)
    seed = np.argwhere(cls != ref.BLOCKED)[0, ::-1]
    full = ref.route(cls, [seed], 26, (10, 14, 17), (8, 3))
    assert full["summary"][2] > 200
    for mc in (1, 10, 57, 200):
        exp = compare(run, obs, 3, [seed], 26, (10, 14, 17), (8, 3), max_cost=mc, tiles=[DEFAULT_TILE, (4, 4, 4), (1, 5, 3)], what=f"max_cost {mc}")
        assert np.array_equal(exp["cost"], np.where(full["cost"] <= mc, full["cost"], -1))
        assert exp["summary"][2] <= mc


def test_serpentine(driver):
    """optimal paths many times the box edge: every tile is entered again and again"""
    _, run = driver
    slab = reach_ref.serpentine_slab(64, 64)
    for conn in (6, 26):
        exp = compare(run, grow(slab), 1, [(0, 0, 0)], conn, (10, 14, 17), (), what="slab")
        assert exp["summary"][2] >= 10 * 20 * 64 and exp["summary"][0] == exp["summary"][1]


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_knob_ranges():
    from mlmapping_amd.mlmap import load_library

    L = load_library()
    try:
        for T in TILES + [(1, 1, 1), (22, 22, 22), (64, 13, 13)]:
            assert L.mlm_debug_set(b"route_tile", pack(T)) == 0, T
        for v in (0, -1, pack((0, 8, 8)), pack((65, 1, 1)), pack((64, 64, 64)), pack((23, 23, 23)) + (1 << 24), 1 << 24, 1 << 40):
            assert L.mlm_debug_set(b"route_tile", v) == -1, v
        for v in (1, 8, 64, GROUP_MAX):
            assert L.mlm_debug_set(b"route_group", v) == 0, v
        for v in (0, -1, GROUP_MAX + 1, 1 << 40):
            assert L.mlm_debug_set(b"route_group", v) == -1, v
    finally:
        L.mlm_debug_reset()


def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_ROUTE_OCC, mlmap.MLM_ROUTE_INFL, mlmap.MLM_ROUTE_UNKNOWN, mlmap.MLM_ROUTE_NONE, mlmap.MLM_ROUTE_SEED) == (1, 2, 4, -1, 26)
    assert callable(mlmap.MLMap.export_route) and callable(mlmap.MLMap.export_route_dev)
    assert "mlm_export_route" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_route")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("OCC", "1"), ("INFL", "2"), ("UNKNOWN", "4"), ("NONE", r"\(-1\)"), ("SEED", "26")):
        assert re.search(rf"#define MLM_ROUTE_{name} {v}(\s|$)", hdr), name
    assert re.search(r"#define MLM_ABI_VERSION 6(\s|$)", hdr)
    assert "exportRoute" in open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
    assert (ref.NONE, ref.SEED) == (mlmap.MLM_ROUTE_NONE, mlmap.MLM_ROUTE_SEED)
