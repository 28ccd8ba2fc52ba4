"""mlm_export_clusters on the CPU: its planner, its per-voxel rules in the device's phase order, and its interface.

* mlm_cluster_plan (mlmapping_amd/csrc/mlm_host.h) built with g++ -fsanitize=address,undefined: the tile grid covers the box exactly
  (the box list of tests/test_reach_plan.py), the scratch bytes match the formula restated here, refused arguments are refused.
* the rules of mlmapping_amd/csrc/mlm_cluster.h (neighbour offsets, local step, find / union, numbering, row start and update: the
  code the kernels run) driven phase by phase, sequentially, on masks generated here: labels, table and summary[0..4] equal the
  breadth-first ground truth (tests/cluster_ref.py) for the three connectivities and several tile geometries.
* the knob's range, the binding's methods and constants."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cluster_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
HALO_VOXELS, CHUNK, CTRL_BYTES = 15360, 2048, 256  # (mlm_host.h kReachHaloVoxels, kClusterChunk, kClusterCtrlBytes)


def pack(t):
    return t[0] | t[1] << 8 | t[2] << 16


DEFAULT_TILE = (32, 8, 8)
TILES = [DEFAULT_TILE, (1, 5, 3), (4, 4, 4), (7, 1, 2), (64, 2, 1)]
CONNS = [6, 18, 26]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cp")
    exe = d / "cluster_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "cluster_driver.cpp"), "-o", str(exe)])

    def plan(*cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(exe), "plan", *args], check=True, capture_output=True, text=True).stdout
        return [[int(x) for x in line.split()] for line in out.splitlines()]

    def run(S, tile, connectivity, min_size=1, cap=0, lo=(0, 0, 0)):
        dz, dy, dx = S.shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([dx, dy, dz, pack(tile), connectivity, min_size, cap, *lo], dtype=np.int64).tobytes())
            f.write(np.ascontiguousarray(S, dtype=np.uint8).tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:64], dtype=np.int64)
        n = dx * dy * dz
        return {"summary": head[:6], "tiles": int(head[6]), "unions": int(head[7]),
                "labels": np.frombuffer(raw[64:64 + 4 * n], dtype=np.int32).reshape(dz, dy, dx),
                "table": np.frombuffer(raw[64 + 4 * n:], dtype=np.int64).reshape(cap, 16)}

    return plan, run


def up(v):
    return (v + 255) // 256 * 256


# ---- the planner --------------------------------------------------------------------------------------------------------------
def test_plan_grid_and_scratch(driver):
    plan, _ = driver
    boxes = [(1, 1, 1), (33, 9, 9), (32, 8, 8), (31, 7, 1), (1, 200, 3), (93, 73, 63), (512, 512, 64), (2 ** 31 - 1, 1, 1), (1, 1, 2 ** 31 - 1),
             (65536, 32767, 1), (1290, 1290, 1290)]
    cases = [(*D, pack(T), fr, cap) for D in boxes for T in TILES for fr, cap in ((0, 0), (1, 1000))]
    rows = plan(*cases)
    assert len(rows) == len(cases)
    for r, c in zip(rows, cases):
        D, tile, fr, cap = c[:3], c[3], c[4], c[5]
        assert tuple(r[:6]) == tuple(c) and r[6] == 1
        T, n, tiles, vox, chunks = r[7:10], r[10:13], r[13], r[14], r[15]
        assert tuple(T) == (tile & 255, tile >> 8 & 255, tile >> 16)
        # the grid covers the box exactly: the last tile per axis starts inside the box and ends at or beyond its edge
        assert all((n[a] - 1) * T[a] < D[a] <= n[a] * T[a] for a in range(3))
        assert tiles == n[0] * n[1] * n[2] and vox == D[0] * D[1] * D[2] and chunks == (vox + CHUNK - 1) // CHUNK
        parts = [up(4 * vox), up(4 * vox), up(vox), up((D[0] + 2) * (D[1] + 2) * (D[2] + 2)) if fr else 0, up(4 * chunks), up(128 * cap)]
        assert r[16:22] == parts
        offs = np.cumsum(parts).tolist()
        assert r[22:28] == offs and r[28] == offs[-1] + CTRL_BYTES
        assert T[0] * T[1] * T[2] < HALO_VOXELS  # (the tile's labels fit the LDS k_reach_sweep's halo box fits)


def test_plan_tiles_cover_each_voxel_once(driver):
    plan, _ = driver
    for D in [(33, 9, 9), (5, 1, 7), (70, 3, 2)]:
        for T in TILES:
            n = plan((*D, pack(T), 0, 0))[0][10:13]
            cover = np.zeros(D[::-1], dtype=np.int32)
            for t2 in range(n[2]):
                for t1 in range(n[1]):
                    for t0 in range(n[0]):
                        cover[t2 * T[2]:(t2 + 1) * T[2], t1 * T[1]:(t1 + 1) * T[1], t0 * T[0]:(t0 + 1) * T[0]] += 1
            assert (cover == 1).all(), (D, T)


def test_plan_refusals(driver):
    plan, _ = driver
    bad_tiles = [0, pack((0, 8, 8)), pack((8, 0, 8)), pack((8, 8, 0)), pack((65, 1, 1)), pack((64, 64, 64)), pack((30, 30, 30)), 1 << 24, -1]
    cases = [(4, 4, 4, t, 0, 0) for t in bad_tiles]
    cases += [(0, 4, 4, pack(DEFAULT_TILE), 0, 0), (4, -1, 4, pack(DEFAULT_TILE), 1, 0), (4, 4, 4, pack(DEFAULT_TILE), 0, -1)]
    assert all(r[6] == 0 for r in plan(*cases))
    assert all(r[6] == 1 for r in plan((4, 4, 4, pack((22, 22, 22)), 1, 1), (4, 4, 4, pack((64, 13, 13)), 0, 0)))


# ---- the rules in the device's phase order ------------------------------------------------------------------------------------
def compare(run, S, conns=CONNS, tiles=TILES, min_sizes=(1,), lo=(0, 0, 0), what=""):
    """labels / table / summary[0..4] of the driver against the ground truth; cap 0, 1, K, K + 1 on the first tile, K + 1 on the others"""
    out = {}
    for conn in conns:
        for ms in min_sizes:
            exp = ref.clusters(S, conn, ms, None, lo)
            K = int(exp["summary"][2])
            out[conn, ms] = exp
            for T in tiles:
                for cap in sorted({0, 1, K, K + 1}) if T == tiles[0] else [K + 1]:
                    got = run(S, T, conn, ms, cap, lo)
                    tag = (what, conn, ms, T, cap)
                    assert np.array_equal(got["labels"], exp["labels"]), tag
                    assert np.array_equal(got["summary"][:5], exp["summary"]), tag
                    rows = min(K, cap)
                    assert np.array_equal(got["table"][:rows], exp["table"][:rows]), tag
                    assert not got["table"][rows:].any(), tag
                    assert (got["summary"][5] >= 1) == bool(S.any()), tag
    return out


@pytest.mark.parametrize("density", [0.1, 0.3, 0.5, 0.9])
def test_random_masks(driver, density):
    """densities around the percolation thresholds of the three connectivities; boxes that are no multiple of any tile"""
    _, run = driver
    rng = np.random.default_rng(int(density * 100))
    for shape in [(7, 19, 37), (1, 40, 33), (12, 1, 50)]:
        S = rng.random(shape) < density
        compare(run, S, min_sizes=(1, 2, 50), lo=(-17, 3, -2 ** 31), what=f"random {density} {shape}")


def test_serpentine_is_one_component(driver):
    """one component through every tile, many times the box edge long"""
    _, run = driver
    S = ~ref.serpentine_3d(16)
    exp = compare(run, S, tiles=[(4, 4, 4), (1, 5, 3), DEFAULT_TILE], min_sizes=(1, 50), what="serpentine")
    for (conn, _), e in exp.items():
        if conn == 6:
            assert tuple(e["summary"]) == (S.sum(), 1, 1, S.sum(), S.sum())
            assert e["table"][0, 13] == 63 and tuple(e["table"][0, 1:4]) == (0, 0, 0)
    walls = ref.serpentine_3d(12)  # the complement: walls that 26-connect
    compare(run, walls, tiles=[(4, 4, 4), (7, 1, 2)], what="serpentine walls")


def test_checkerboard(driver):
    _, run = driver
    for shape in [(6, 9, 11), (2, 2, 2), (1, 7, 5), (1, 1, 9)]:
        S = ref.checkerboard(shape)
        exp = compare(run, S, tiles=[(4, 4, 4), (1, 5, 3), (7, 1, 2)], min_sizes=(1, 2), what=f"checkerboard {shape}")
        assert exp[6, 1]["summary"][1] == S.sum() and exp[6, 1]["summary"][4] == 1 and exp[6, 2]["summary"][2] == 0
        assert (exp[6, 2]["labels"][S] == ref.SMALL).all()
        if min(shape) >= 2:
            assert exp[18, 1]["summary"][1] == 1


def test_corner_contact_across_a_tile_corner(driver):
    """two voxels that touch only by a corner, on either side of a tile corner: one component at 26 only"""
    _, run = driver
    for T in TILES:
        S = np.zeros((2 * T[2] + 1, 2 * T[1] + 1, 2 * T[0] + 1), dtype=bool)
        S[T[2] - 1, T[1] - 1, T[0] - 1] = S[T[2], T[1], T[0]] = True
        exp = compare(run, S, tiles=[T], min_sizes=(1, 2), what=f"corner {T}")
        joined = exp[26, 1]["labels"][T[2] - 1, T[1] - 1, T[0] - 1] == exp[26, 1]["labels"][T[2], T[1], T[0]]
        assert joined and exp[18, 1]["labels"][T[2] - 1, T[1] - 1, T[0] - 1] != exp[18, 1]["labels"][T[2], T[1], T[0]]
        # ... and by an edge across a tile edge: 18 and 26, not 6
        S = np.zeros_like(S)
        S[0, T[1] - 1, T[0] - 1] = S[0, T[1], T[0]] = True
        exp = compare(run, S, tiles=[T], what=f"edge {T}")
        assert [int(exp[c, 1]["summary"][1]) for c in CONNS] == [2, 1, 1]


def test_empty_full_and_one_voxel(driver):
    _, run = driver
    for shape in [(5, 9, 34), (1, 1, 1)]:
        exp = compare(run, np.zeros(shape, dtype=bool), what="empty")
        assert not exp[6, 1]["summary"].any() and (exp[6, 1]["labels"] == ref.NONE).all()
        full = np.ones(shape, dtype=bool)
        exp = compare(run, full, min_sizes=(1, 2, 50), lo=(2 ** 31 - 1 - shape[2], -5, 0), what="full")
        n = full.size
        assert tuple(exp[6, 1]["summary"]) == (n, 1, 1, n, n) and (exp[6, 1]["labels"] == 0).all()
        assert exp[6, 1]["table"][0, 13] == 63


def test_reference_forms_agree():
    """the breadth-first ground truth against scipy's labelling (where scipy imports; labels up to a permutation there) and the
    frontier set against the definition taken voxel by voxel"""
    rng = np.random.default_rng(3)
    S = rng.random((9, 14, 17)) < 0.35
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for conn, rank in ((6, 1), (18, 2), (26, 3)):
        comp, n = ref.components(S, conn)
        assert (comp >= 0).sum() == S.sum() and n == len(np.unique(comp[S]))
        first = [np.flatnonzero(comp.ravel() == k)[0] for k in range(n)]
        assert first == sorted(first)  # root order
        if ndimage is not None:
            lab, m = ndimage.label(S, structure=ndimage.generate_binary_structure(3, rank))
            assert m == n and len(np.unique(np.stack([lab[S], comp[S]]), axis=1).T) == n
    occ = rng.integers(-1, 2, size=(6, 7, 8))
    F = ref.frontier_set(occ)
    for z in range(4):
        for y in range(5):
            for x in range(6):
                c = (z + 1, y + 1, x + 1)
                nb = [occ[c[0] + a, c[1] + b, c[2] + d] for a, b, d in ref.offsets(6)]
                assert F[z, y, x] == (occ[c] == 1 and -1 in nb)


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_knob_range():
    from mlmapping_amd.mlmap import load_library

    L = load_library()
    try:
        for T in TILES + [(1, 1, 1), (22, 22, 22), (64, 13, 13)]:
            assert L.mlm_debug_set(b"cluster_tile", pack(T)) == 0, T
        for v in (0, -1, pack((0, 8, 8)), pack((65, 1, 1)), pack((64, 64, 64)), pack((23, 23, 23)) + (1 << 24), 1 << 24, 1 << 40):
            assert L.mlm_debug_set(b"cluster_tile", v) == -1, v
    finally:
        L.mlm_debug_reset()


def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_CLUSTER_OCC, mlmap.MLM_CLUSTER_INFL, mlmap.MLM_CLUSTER_UNKNOWN, mlmap.MLM_CLUSTER_FRONTIER) == (1, 2, 4, 16)
    assert (mlmap.MLM_CLUSTER_NONE, mlmap.MLM_CLUSTER_SMALL, mlmap.MLM_CLUSTER_ROW) == (ref.NONE, ref.SMALL, ref.ROW) == (-1, -2, 16)
    assert callable(mlmap.MLMap.export_clusters) and callable(mlmap.MLMap.export_clusters_dev)
    assert "mlm_export_clusters" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_clusters")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("OCC", "1"), ("INFL", "2"), ("UNKNOWN", "4"), ("FRONTIER", "16"), ("NONE", r"\(-1\)"), ("SMALL", r"\(-2\)"), ("ROW", "16")):
        assert re.search(rf"#define MLM_CLUSTER_{name} {v}(\s|$)", hdr), name
    assert re.search(r"#define MLM_ABI_VERSION 6(\s|$)", hdr)
