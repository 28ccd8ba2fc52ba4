"""mlm_export_octree on the CPU: its planner, its rules in the device's phase order, its file format and its interface.

* mlm_oct_plan / mlm_oct_args (mlmapping_amd/csrc/mlm_octree.h) built with g++ -fsanitize=address,undefined: the scratch bytes match
  the formula restated here, refused arguments are refused.
* the rules of mlm_octree.h (class -> label, the eight-children reduction, child order, subtree counts, the hand-down of numbers, the
  rows: the code the kernels run) driven phase by phase, sequentially, on class arrays generated here: all five arrays and the summary
  equal the numpy / Python ground truth (tests/octree_ref.py) byte for byte, which is itself checked for the properties of a tree.
* octree_io's to_bt / from_bt round trip and leaves_of; the binding's names and constants."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import octree_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
CTRL_BYTES = 1024  # (mlm_octree.h kOctCtrlBytes)
SENT = 0x77
FLAGS = [0, ref.INFL, ref.OCC_ONLY, ref.INFL | ref.OCC_ONLY]
# dims, lo: one voxel; a box straddling the origin; one crossing brick edges on every axis; a flat strip; a box touching both ends of
# the key cube at depth 7; one that holds the aligned 32^3 cube [-32, 0) x [0, 32) x [0, 32)
BOXES = [((1, 1, 1), (-1, 0, -1)), ((17, 5, 3), (-9, -2, -1)), ((33, 33, 33), (15, -16, 1)), ((64, 2, 1), (-7, 5, 3)),
         ((128, 3, 2), (-64, -1, 0)), ((48, 40, 36), (-40, -4, -2))]
SETS = ["full", "empty", "checkerboard", "random", "uniform"]
KEYS = (("words", 1, np.uint16, 1), ("inner4", 4, np.int32, 2), ("skip", 1, np.int32, 4), ("leaf4", 4, np.int32, 8), ("leaf_class", 1, np.int8, 16))


def smallest_depth(dims, lo):
    d = 1
    while not all(lo[a] >= -(1 << (d - 1)) and lo[a] + dims[a] <= (1 << (d - 1)) for a in range(3)):
        d += 1
    return d


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("op")
    exe = d / "octree_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "octree_driver.cpp"), "-o", str(exe)])

    def lines(mode, *cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(exe), mode, *args], check=True, capture_output=True, text=True).stdout
        return [[int(x) for x in line.split()] for line in out.splitlines()]

    def run(occ, infl, lo, depth, flags, cap_n, cap_m, which=31, step=0):
        dz, dy, dx = occ.shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([dx, dy, dz, *lo, depth, flags, cap_n, cap_m, which, step], dtype=np.int64).tobytes())
            f.write(np.ascontiguousarray(occ, dtype=np.int8).tobytes())
            f.write(np.ascontiguousarray(infl, dtype=np.int8).tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        out, at = {"summary": np.frombuffer(raw[:8 * ref.ROW], dtype=np.int64)}, 8 * ref.ROW
        for key, cols, dt, _ in KEYS:
            rows = cap_n if key in ("words", "inner4", "skip") else cap_m
            size = rows * cols * np.dtype(dt).itemsize
            out[key] = np.frombuffer(raw[at:at + size], dtype=dt).reshape((rows, cols) if cols > 1 else (rows,))
            at += size
        assert at == len(raw)
        return out

    return lines, run


def up(v):
    return (v + 255) // 256 * 256


def cells_per_level(dims, lo, depth):
    half, T = 1 << (depth - 1), min(depth, 4)
    out = []
    for lv in range(T, depth + 1):
        n = 1
        for a in range(3):
            n *= ((lo[a] + dims[a] - 1 + half) >> lv) - ((lo[a] + half) >> lv) + 1
        out.append(n)
    return T, out


# ---- the planner --------------------------------------------------------------------------------------------------------------
def test_plan_scratch(driver):
    lines, _ = driver
    cases = [(dims, lo, dp) for dims, lo in BOXES for dp in (16, smallest_depth(dims, lo), 31)]
    cases += [((512, 512, 64), (-256, -256, -16), 16), ((512, 512, 64), (-250, -251, -3), 16), ((2 ** 31 - 1, 1, 1), (-2 ** 30, 0, 0), 31),
              ((1290, 1290, 1290), (-645, -645, -645), 11), ((2, 2, 2), (-1, -1, -1), 1), ((8, 8, 8), (-4, -4, -4), 3), ((16, 16, 16), (-8, -8, -8), 4),
              ((32, 32, 32), (-16, -16, -16), 5)]
    rows = lines("plan", *[(*lo, *dims, dp) for dims, lo, dp in cases])
    assert len(rows) == len(cases)
    for r, (dims, lo, dp) in zip(rows, cases):
        T, per = cells_per_level(dims, lo, dp)
        C = sum(per)
        assert r[0] == 0 and r[1] == T and r[2] == per[0] and r[3] == C, (dims, lo, dp)
        assert per[-1] == 1  # (the root)
        # a label byte and four int32 per cell of levels T..depth, and the control block
        assert r[4:6] == [up(C), up(4 * C)]
        offs = [up(C) + k * up(4 * C) for k in range(5)]
        assert r[6:11] == offs and r[11] == up(C) + 4 * up(4 * C) + CTRL_BYTES
        assert r[12:] == np.concatenate([[0], np.cumsum(per)]).tolist()
    # 17 bytes per brick and a little: a 512 x 512 x 64 box aligned to the bricks has 32 * 32 * 4 of them
    assert rows[len(BOXES) * 3][2] == 4096 and rows[len(BOXES) * 3][11] < 4096 * 17 * 1.2 + 8192


def test_plan_and_argument_refusals(driver):
    lines, _ = driver
    # lo, dims, depth -> why
    bad = [((0, 0, 0, 1, 1, 1, 0), 1), ((0, 0, 0, 1, 1, 1, 32), 1), ((0, 0, 0, 1, 1, 1, -3), 1), ((0, 0, 0, 0, 1, 1, 16), 2), ((0, 0, 0, 1, -1, 1, 16), 2),
           ((1, 0, 0, 1, 1, 1, 1), 2), ((-2, 0, 0, 1, 1, 1, 1), 2), ((0, 0, -32769, 1, 1, 1, 16), 2), ((0, 32767, 0, 1, 2, 1, 16), 2),
           ((-64, 0, 0, 129, 1, 1, 7), 2), ((-65, 0, 0, 128, 1, 1, 7), 2)]
    assert [r[0] for r in lines("plan", *[b[0] for b in bad])] == [b[1] for b in bad]
    good = [(0, 0, 0, 1, 1, 1, 1), (-1, -1, -1, 2, 2, 2, 1), (0, 32767, 0, 1, 1, 1, 16), (-32768, 0, 0, 65536, 1, 1, 16), (-64, 0, 0, 128, 1, 1, 7),
            (-2 ** 30, 0, 0, 2 ** 31 - 1, 1, 1, 31)]
    assert [r[0] for r in lines("plan", *good)] == [0] * len(good)
    # flags, cap_inner, an inner array given, cap_leaves, a leaf array given, summary given
    good = [(0, 0, 0, 0, 0, 1), (3, 5, 1, 0, 0, 0), (2, 0, 0, 9, 1, 0), (1, 2 ** 40, 1, 2 ** 40, 1, 1), (0, 1, 1, 1, 1, 0)]
    assert [r[0] for r in lines("args", *good)] == [0] * len(good)
    bad = [((4, 0, 0, 0, 0, 1), 1), ((-1, 0, 0, 0, 0, 1), 1), ((1 | 1 << 30, 0, 0, 0, 0, 1), 1), ((16, 0, 0, 0, 0, 1), 1), ((0, -1, 1, 0, 0, 1), 2),
           ((0, 0, 0, -5, 1, 1), 2), ((0, 0, 1, 0, 0, 1), 3), ((0, 4, 0, 0, 0, 1), 3), ((0, 0, 0, 0, 1, 1), 3), ((0, 0, 0, 4, 0, 1), 3), ((0, 0, 0, 0, 0, 0), 4)]
    assert [r[0] for r in lines("args", *[b[0] for b in bad])] == [b[1] for b in bad]


# ---- the rules in the device's phase order ------------------------------------------------------------------------------------
def aligned_cube(dims, lo, kmax=5):
    """the largest cube of side 2^k <= 32 on the lattice of multiples of its side that lies in the box: (corner in box coordinates, side)"""
    for k in range(kmax, 0, -1):
        s = 1 << k
        c = [-(-lo[a] // s) * s for a in range(3)]  # the first multiple of s at or above lo
        if all(c[a] + s <= lo[a] + dims[a] for a in range(3)):
            return [c[a] - lo[a] for a in range(3)], s
    return None, 0


def classes(kind, dims, lo, rng, turn):
    shape = (dims[2], dims[1], dims[0])
    if kind == "full":
        occ, infl = np.full(shape, turn % 2, dtype=np.int8), np.full(shape, -1, dtype=np.int8)
    elif kind == "empty":
        occ, infl = np.full(shape, -1, dtype=np.int8), np.full(shape, -1, dtype=np.int8)
    elif kind == "checkerboard":
        occ, infl = (np.indices(shape).sum(axis=0) % 2).astype(np.int8), np.full(shape, -1, dtype=np.int8)
    else:
        p = [0.2, 0.5, 0.3] if kind == "random" else [0.05, 0.9, 0.05]
        occ = rng.choice(np.array([0, 1, -1], dtype=np.int8), size=shape, p=p)
        infl = np.where(rng.random(shape) < 0.15, 0, -1).astype(np.int8)
    if kind == "uniform":
        c, s = aligned_cube(dims, lo)
        if s:
            occ[c[2]:c[2] + s, c[1]:c[1] + s, c[0]:c[0] + s] = 1 - turn % 2
            infl[c[2]:c[2] + s, c[1]:c[1] + s, c[0]:c[0] + s] = -1
    return occ, infl


def compare(got, exp, cap_n, cap_m, which, tag):
    N, M = int(exp["summary"][0]), int(exp["summary"][1])
    assert np.array_equal(got["summary"], exp["summary"]), (tag, got["summary"], exp["summary"])
    for key, _, _, bit in KEYS:
        total, cap = (N, cap_n) if key in ("words", "inner4", "skip") else (M, cap_m)
        rows = min(total, cap) if which & bit else 0
        g = got[key]
        assert g[:rows].tobytes() == exp[key][:rows].tobytes(), (tag, key)
        assert (np.frombuffer(g[rows:].tobytes(), dtype=np.uint8) == SENT).all(), (tag, key, "rows beyond the cap were written")


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(map(str, b[0])))
def test_rules_against_numpy(driver, box):
    """every set at depth 16 and at the smallest depth that fits: the random sets at depth 16 with every flag combination, the others
    with a rotating one; the caps, ranges of rows and subsets of the arrays on every fourth case"""
    _, run = driver
    dims, lo = box
    rng = np.random.default_rng(sum(dims))
    turn = 0
    for kind in (SETS if dims != (48, 40, 36) else ["random", "uniform"]):  # (the largest box is there for the 32^3 cube)
        for depth in (16, smallest_depth(dims, lo)):
            for flags in (FLAGS if depth == 16 and kind in ("random", "uniform") else [FLAGS[turn % 4]]):
                occ, infl = classes(kind, dims, lo, rng, turn)
                exp = ref.tree(occ, infl, lo, depth, flags)
                ref.check(exp, depth, lo, dims)
                N, M = int(exp["summary"][0]), int(exp["summary"][1])
                tag = (box, kind, depth, flags)
                if kind == "empty" or (kind == "full" and turn % 2 and flags & ref.OCC_ONLY):
                    assert N == 0 and M == 0 and exp["summary"][6] == ref.NONE
                if kind == "uniform" and aligned_cube(dims, lo)[1] == 32 and not (flags & ref.OCC_ONLY and turn % 2 == 0):
                    assert exp["summary"][8 + 5] == 1, tag  # the aligned 32^3 cube is one level-5 leaf
                compare(run(occ, infl, lo, depth, flags, N + 1, M + 1), exp, N + 1, M + 1, 31, tag)
                if turn % 4 == 0:
                    for cap_n, cap_m in sorted({(0, 0), (1, 1), (max(N - 1, 0), max(M - 1, 0)), (N, M), (0, M), (N, 0)}):
                        compare(run(occ, infl, lo, depth, flags, cap_n, cap_m), exp, cap_n, cap_m, 31, tag + (cap_n, cap_m))
                    compare(run(occ, infl, lo, depth, flags, N + 1, M + 1, step=7), exp, N + 1, M + 1, 31, tag + ("ranges of 7 rows",))
                    compare(run(occ, infl, lo, depth, flags, max(N - 1, 0), M + 1, step=5), exp, max(N - 1, 0), M + 1, 31, tag + ("ranges of 5 rows",))
                    for which in (1, 2, 4, 8, 16, 1 | 16):
                        compare(run(occ, infl, lo, depth, flags, N + 1, M + 1, which=which), exp, N + 1, M + 1, which, tag + ("arrays", which))
                turn += 1


def test_reference_on_cases_known_by_hand():
    """one voxel; a full key cube; eight voxels around the origin"""
    t = ref.tree(np.zeros((1, 1, 1), dtype=np.int8), np.full((1, 1, 1), -1), (0, 0, 0), 2, 0)
    # depth 2: keys 0..3, the voxel has key 2: child 7 of the root (level 1, corner 0), there child 0
    assert t["words"].tolist() == [3 << 14, 2] and t["inner4"].tolist() == [[-2, -2, -2, 2], [0, 0, 0, 1]] and t["skip"].tolist() == [2, 2]
    assert t["leaf4"].tolist() == [[0, 0, 0, 0]] and t["leaf_class"].tolist() == [0]
    assert t["summary"].tolist()[:9] == [2, 1, 1, 0, 1, 0, ref.INNER, 0, 1]
    t = ref.tree(np.ones((4, 4, 4), dtype=np.int8), np.full((4, 4, 4), -1), (-2, -2, -2), 2, 0)
    assert len(t["words"]) == 0 and t["leaf4"].tolist() == [[-2, -2, -2, 2]] and t["leaf_class"].tolist() == [1]
    assert t["summary"].tolist()[:8] == [0, 1, 0, 1, 0, 64, ref.FREE, 0] and t["summary"][8 + 2] == 1
    ref.check(t, 2, (-2, -2, -2), (4, 4, 4))
    occ = np.zeros((2, 2, 2), dtype=np.int8)
    t = ref.tree(occ, np.full(occ.shape, -1), (-1, -1, -1), 3, 0)  # eight voxels around the origin: one in each child of the root
    assert len(t["words"]) == 1 + 8 + 8 and t["words"][0] == 0xFFFF and len(t["leaf4"]) == 8 and (t["leaf4"][:, 3] == 0).all()
    assert t["leaf4"][0].tolist() == [-1, -1, -1, 0] and t["leaf4"][7].tolist() == [0, 0, 0, 0]
    ref.check(t, 3, (-1, -1, -1), (2, 2, 2))


# ---- the file format ----------------------------------------------------------------------------------------------------------
def test_bt_round_trip_and_leaves():
    from mlmapping_amd import octree_io as io

    rng = np.random.default_rng(5)
    dims, lo = (21, 18, 9), (-9, 3, -4)
    occ, infl = classes("random", dims, lo, rng, 0)
    occ[0:8, 8:16, 0:8] = 1  # (some pruned cubes)
    for depth in (16, 6):
        t = ref.tree(occ, infl, lo, depth, 0)
        data = io.to_bt(t["words"], len(t["leaf4"]), 0.05)
        head = data[:data.index(b"data\n")].decode("ascii").splitlines()
        assert head[0] == "# Octomap OcTree binary file" and head[-3:] == ["id OcTree", f"size {len(t['words']) + len(t['leaf4'])}", "res 0.05"]
        assert all(line.startswith("#") for line in head[1:-3])
        assert data[data.index(b"data\n") + 5:] == t["words"].astype("<u2").tobytes()
        back = io.from_bt(data)
        assert back["words"].dtype == np.uint16 and np.array_equal(back["words"], t["words"])
        assert back["size"] == len(t["words"]) + len(t["leaf4"]) and back["res"] == 0.05 and back["id"] == "OcTree"
        leaf4, leaf_class = io.leaves_of(back["words"], depth)
        assert leaf4.dtype == np.int32 and leaf_class.dtype == np.int8
        assert np.array_equal(leaf4, t["leaf4"]) and np.array_equal(leaf_class, t["leaf_class"])
    empty = io.from_bt(io.to_bt(np.zeros(0, dtype=np.uint16), 0, 0.1))
    assert len(empty["words"]) == 0 and empty["size"] == 0 and len(io.leaves_of(empty["words"], 16)[0]) == 0
    for bad in (b"# something else\n", io.to_bt([3], 1, 0.1)[:-1], b"# Octomap OcTree binary file\nid OcTree\nres 0.1\ndata\n"):
        with pytest.raises(ValueError):
            io.from_bt(bad)
    for bad in ([0xFFFF], [3, 2, 2]):  # the stream ends inside the tree; words left over
        with pytest.raises(ValueError):
            io.leaves_of(np.array(bad, dtype=np.uint16), 4)
    assert "UNPINNED" in io.__doc__


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_OCT_INFL, mlmap.MLM_OCT_OCC_ONLY, mlmap.MLM_OCT_ROW) == (1, 2, 40) == (ref.INFL, ref.OCC_ONLY, ref.ROW)
    assert (mlmap.MLM_OCT_NONE, mlmap.MLM_OCT_FREE, mlmap.MLM_OCT_OCC, mlmap.MLM_OCT_INNER) == (0, 1, 2, 3) == (ref.NONE, ref.FREE, ref.OCC, ref.INNER)
    assert callable(mlmap.MLMap.export_octree) and callable(mlmap.MLMap.export_octree_dev)
    assert "mlm_export_octree" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_octree")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("INFL", "1"), ("OCC_ONLY", "2"), ("ROW", "40")):
        assert re.search(rf"#define MLM_OCT_{name} {v}(\s|$)", hdr), name
    assert re.search(r"#define MLM_ABI_VERSION 6(\s|$)", hdr)
    assert re.search(r"\bvoid octree\(", open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read())
