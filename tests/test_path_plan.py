"""mlm_query_paths on the CPU: its rule, its reference and its interface.

* tests/path_ref.py held to properties first: vis is symmetric, contains tests/raywalk_ref.py's path between the voxel centres,
  equals tests/route_ref.py's permitted-move rule for unit offsets; every way-point leg of every answer is visible or a single move;
  lookahead 1 returns route_ref.walk; a 6-connected unit-cost route field and the reach field give the same paths.
* mlmapping_amd/csrc/mlm_path.h (the code the kernel and the entry point's host branch run) built as a stand-alone program with
  g++ -fsanitize=address,undefined and run on the cases of tests/path_cases.py: every output byte for byte the reference's, length by
  its 64 bits; vis on random pairs, tie groups included.
* non-vacuity of those cases, asserted on the reference's answers; the binding's constants, signatures and host-side refusals."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import path_cases as pc
from tests import path_ref as ref
from tests import raywalk_ref, reach_ref, route_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("path")
    exe = d / "path_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "path_driver.cpp"), "-o", str(exe)])

    def header(f, parent, lo, kind, n, L, mm, cap):
        dz, dy, dx = parent.shape
        f.write(np.array([dx, dy, dz, *lo, kind, n, L, mm, cap], dtype=np.int32).tobytes())
        f.write(np.float64(np.float32(pc.D_SUB)).tobytes())
        f.write(np.ascontiguousarray(parent, dtype=np.uint8).tobytes())

    def run(c):
        n, cap = len(c["goals"]), c["cap"]
        with open(d / "in.bin", "wb") as f:
            header(f, c["parent"], c["lo"], c["kind"], n, c["lookahead"], c["max_moves"], cap)
            f.write(c["goals"].tobytes())
            f.write(c["fill"].tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        assert len(raw) == n * (1 + 12 * cap + 8 + 64)
        o = [0, n, n + 12 * n * cap, n + 12 * n * cap + 8 * n]
        return {"status": np.frombuffer(raw[:o[1]], dtype=np.int8), "way": np.frombuffer(raw[o[1]:o[2]], dtype=np.int32).reshape(n, cap, 3),
                "length": np.frombuffer(raw[o[2]:o[3]], dtype=np.float64), "table": np.frombuffer(raw[o[3]:], dtype=np.int64).reshape(n, 8)}

    def pairs(parent, kind, ab):
        ab = np.ascontiguousarray(ab, dtype=np.int32).reshape(-1, 6)
        with open(d / "in.bin", "wb") as f:
            header(f, parent, (0, 0, 0), kind, len(ab), 1, 1, 0)
            f.write(ab.tobytes())
        subprocess.run([str(exe), "pairs", str(d / "in.bin"), str(d / "out.bin")], check=True)
        return np.frombuffer(open(d / "out.bin", "rb").read(), dtype=np.uint8)

    return run, pairs


# ---- the reference held to properties -----------------------------------------------------------------------------------------
def cube_pairs(seed=5, n=9, count=2000, density=0.1):
    rng = np.random.default_rng(seed)
    parent = np.where(rng.random((n, n, n)) < density, 255, 0).astype(np.uint8)
    free = np.argwhere(parent == 0)[:, ::-1]
    return parent, free[rng.integers(len(free), size=count)], free[rng.integers(len(free), size=count)]


def test_vis_symmetric_and_contains_the_ray_path():
    parent, A, B = cube_pairs()
    F = ref.Field(parent, ref.ROUTE)
    seen, n_vis = set(), 0
    for a, b in zip(A.tolist(), B.tolist()):
        v = ref.vis(F, a, b, seen)
        assert v == ref.vis(F, b, a), (a, b)
        n_vis += v
        tested = {tuple(a)} | {x for _, vox in ref.walk_sets(a, b) for x in vox}
        ray, _ = raywalk_ref.path([1024 * x + 512 for x in a], [1024 * x + 512 for x in b])
        assert {vox for vox, _ in ray} <= tested, (a, b)
        assert tuple(b) in tested
    assert seen == {2, 3} and 200 < n_vis < 1800


def test_vis_of_unit_offsets_is_the_permitted_move():
    rng = np.random.default_rng(9)
    T = rng.random((5, 6, 7)) > 0.3
    F = ref.Field(np.where(T, 0, 255).astype(np.uint8), ref.ROUTE)
    some = 0
    for o in ref.OFFSETS:
        ok = route_ref.permitted(T, o)
        for z, y, x in np.argwhere(T):
            b = (x + o[0], y + o[1], z + o[2])
            if F.open(b):
                assert ref.vis(F, (x, y, z), b) == bool(ok[z, y, x]), (o, x, y, z)
                some += not ok[z, y, x]
            else:
                assert not ok[z, y, x]
    assert some > 50  # (refused diagonals between open voxels: the corner rule, not the end points, decides)


def test_ties_refuse_what_the_ray_walk_passes():
    by_name = {c["name"]: c for c in pc.build()}
    for name, a, b in (("hand-tie2-closed", (2, 2, 0), (0, 0, 0)), ("hand-tie3-one-closed", (1, 1, 1), (0, 0, 0))):
        F = ref.Field(by_name[name]["parent"], ref.ROUTE)
        ray, ties = raywalk_ref.path([1024 * x + 512 for x in a], [1024 * x + 512 for x in b])
        assert ties and all(F.open(v) for v, _ in ray)  # mlm_query_rays' own path is open all the way
        assert not ref.vis(F, a, b) and not ref.vis(F, b, a)
        F_open = ref.Field(by_name[name.replace("one-closed", "open").replace("closed", "open")]["parent"], ref.ROUTE)
        assert ref.vis(F_open, a, b)


def test_answers_are_sound():
    """every leg visible or a single move; way points, counts and table consistent with the raw path; lookahead 1 is the raw walk"""
    for c in pc.build():
        a = pc.answer(c)
        F = ref.Field(c["parent"], c["kind"])
        walk = route_ref.walk if c["kind"] == ref.ROUTE else reach_ref.walk
        for i, det in enumerate(a["detail"]):
            if det is None:
                assert a["status"][i] != 1 and a["length"][i] == -1.0 and (a["table"][i, 1:] == 0).all()
                assert (a["way"][i] == c["fill"][i]).all()
                continue
            path, idx = det
            K, L = len(path) - 1, c["lookahead"]
            assert idx[0] == 0 and idx[-1] == K and a["table"][i, 0] == K and a["table"][i, 1] == len(idx)
            assert a["table"][i, 2:5].sum() == K
            for s, t in zip(idx[:-1], idx[1:]):
                assert s < t <= s + L and (t == s + 1 or ref.vis(F, path[s], path[t]))
            if L == 1:
                assert idx == list(range(K + 1))
                if c["group"] == "random" and "corrupt" not in c["name"]:
                    g = tuple(int(c["goals"][i, x]) - int(c["lo"][x]) for x in range(3))
                    assert [tuple(p) for p in walk(c["parent"], g)] == path
            assert (a["way"][i, len(idx):] == c["fill"][i, len(idx):]).all()


def test_reach_and_unit_route_give_the_same_paths():
    rng = np.random.default_rng(3)
    T = rng.random((5, 14, 19)) > 0.25
    seeds = np.argwhere(T)[[4, 300], ::-1]
    a = route_ref.route(np.where(T, 0, route_ref.BLOCKED).astype(np.uint8), seeds, 6, (1, 1, 1), ())["parent"]
    b = reach_ref.reach(T, seeds)["parent"]
    goals = np.argwhere(b <= 6)[::5, ::-1]
    for L in (1, 3, 16):
        x = ref.query(a, ref.ROUTE, (0, 0, 0), goals, L, 4096, 8, pc.D_SUB)
        y = ref.query(b, ref.REACH, (0, 0, 0), goals, L, 4096, 8, pc.D_SUB)
        pc.assert_same(x, y, L)
        assert (x["status"] == 1).all() and (x["table"][:, 3:5] == 0).all()


def test_cases_are_not_vacuous():
    cases = pc.build()
    for c in cases:
        pc.answer(c)
    rnd = [c for c in cases if c["group"] == "random"]
    st = np.concatenate([pc.answer(c)["status"] for c in rnd])
    assert set(st.tolist()) == {1, 0, -1, -2}
    tab = np.concatenate([pc.answer(c)["table"][pc.answer(c)["status"] == 1] for c in rnd if c["lookahead"] == 16 and c["max_moves"] == 4096])
    assert len(tab) > 300
    assert 3 * (tab[:, 1] < tab[:, 0] + 1).sum() >= len(tab)
    assert 3 * (tab[:, 6] > 0).sum() >= len(tab)
    assert pc.stats["random"]["ties"] == {2, 3}
    tested, refused = pc.stats["random"]["counts"]
    assert refused > tested // 4 and tested - refused > tested // 20
    assert max(pc.answer(c)["table"][:, 0].max() for c in cases if c["group"] == "maze") > 256
    assert max(pc.answer(c)["table"][:, 5].max() for c in cases if c["group"] == "slab") > 64
    # the straight run of the slab: legs reach the full window, W = ceil(K / L) + 1
    for c in cases:
        if c["group"] == "slab":
            row = pc.answer(c)["table"][0]
            assert row[0] == 199 and row[1] == -(-199 // c["lookahead"]) + 1 and row[5] == min(199, c["lookahead"])
    # the maze's far goal at max_moves K - 1, K, K + 1
    assert [int(pc.answer(c)["status"][0]) for c in cases if c["name"].startswith("maze-mm")] == [-1, 1, 1]
    hand = np.concatenate([pc.answer(c)["status"] for c in cases if c["group"] == "hand"])
    assert set(hand.tolist()) == {1, 0, -1, -2}
    assert [int(pc.answer(c)["table"][0, 1]) for c in cases if c["name"].startswith("hand-tie")] == [2, 3, 4, 2, 3]


# ---- the shared rule under the sanitizers -------------------------------------------------------------------------------------
def test_driver_vis_pairs(driver):
    _, pairs = driver
    parent, A, B = cube_pairs(seed=6)
    F = ref.Field(parent, ref.ROUTE)
    got = pairs(parent, ref.ROUTE, np.concatenate([A, B], axis=1))
    groups = 0
    for a, b, g in zip(A.tolist(), B.tolist(), got.tolist()):
        seen = set()
        assert (g & 1) == ref.vis(F, a, b, seen), (a, b)
        assert g >> 1 == (1 if 2 in seen else 0) | (2 if 3 in seen else 0), (a, b)
        groups |= g >> 1
    assert groups == 3
    # far pairs in an open box: the longest walks the contract allows
    big = np.zeros((2, 3, 4097), dtype=np.uint8)
    assert pairs(big, ref.ROUTE, [[0, 0, 0, 4096, 2, 1], [4096, 0, 1, 0, 2, 0], [0, 1, 0, 4096, 1, 0]]).tolist() == [1, 1, 1]


@pytest.mark.parametrize("group", ["random", "maze", "slab", "hand", "cap"])
def test_driver_equals_reference(driver, group):
    run, _ = driver
    cases = [c for c in pc.build() if c["group"] == group]
    assert cases
    for c in cases:
        pc.assert_same(run(c), pc.answer(c), c["name"])


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_PATH_REACH, mlmap.MLM_PATH_ROUTE, mlmap.MLM_PATH_ROW) == (0, 1, 8) == (ref.REACH, ref.ROUTE, ref.ROW)
    assert "mlm_query_paths" in mlmap.ABI_SYMBOLS and hasattr(mlmap.load_library(), "mlm_query_paths")
    sig = inspect.signature(mlmap.MLMap.query_paths)
    assert list(sig.parameters)[1:] == ["lo", "dims", "parent", "goals", "kind", "lookahead", "max_moves", "cap", "outputs"]
    assert [sig.parameters[k].default for k in ("kind", "lookahead", "max_moves", "cap", "outputs")] == ["route", 64, None, 64, None]
    assert list(inspect.signature(mlmap.MLMap.route_paths).parameters)[1:5] == ["lo", "dims", "seeds", "goals"]
    assert callable(mlmap.MLMap.query_paths_dev)
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("REACH", "0"), ("ROUTE", "1"), ("ROW", "8")):
        assert re.search(rf"#define MLM_PATH_{name} {v}(\s|$)", hdr), name
    assert re.search(r"#define MLM_ABI_VERSION 6(\s|$)", hdr)
    facade = open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()
    assert "queryPaths" in facade and "tracePath" in facade
    assert mlmap.MLMap._path_max_moves((512, 512, 64), None) == 8 * 1088 and mlmap.MLMap._path_max_moves((1, 1, 1), None) == 1
    assert mlmap.MLMap._path_max_moves((3, 2, 2), None) == 11 and mlmap.MLMap._path_max_moves((4096, 4096, 100), None) == 66336


def test_refusals_without_a_handle():
    """arguments the binding refuses before the library is called, and the library's answer to a null handle"""
    from mlmapping_amd import mlmap

    m = object.__new__(mlmap.MLMap)  # (no handle: nothing below may reach the library)
    parent, goals = np.zeros((2, 3, 4), dtype=np.uint8), np.zeros((1, 3), dtype=np.int32)
    for kw in ({"outputs": ()}, {"outputs": ("status", "nope")}, {"kind": "astar"}, {"kind": 2}, {"cap": -1}, {"cap": 0}):
        with pytest.raises(mlmap.MlmError):
            m.query_paths((0, 0, 0), (4, 3, 2), parent, goals, **kw)
    with pytest.raises(mlmap.MlmError):
        m.query_paths((0, 0, 0), (4, 3, 3), parent, goals)   # not one byte per voxel
    with pytest.raises(mlmap.MlmError):
        m.query_paths((0, 0, 0), (4, 0, 2), parent, goals)   # the window
    with pytest.raises(mlmap.MlmError):
        m.query_paths_dev((0, 0, 0), (4, 3, 2), 0, 0, 0, kind="x")
    L = mlmap.load_library()
    st = np.zeros(1, dtype=np.int8)
    lo, dims = np.zeros(3, dtype=np.int32), np.array([4, 3, 2], dtype=np.int32)
    assert L.mlm_query_paths(None, mlmap._p(lo), mlmap._p(dims), mlmap._p(parent), 1, mlmap._p(goals), 1, 4, 4, 0, mlmap._p(st), None, None, None) == -1
