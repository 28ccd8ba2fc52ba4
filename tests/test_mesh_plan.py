"""mlm_export_mesh on the CPU: its planner, its rules in the device's phase order, and its interface.

* mlm_mesh_plan / mlm_mesh_args / mlm_mesh_div (mlmapping_amd/csrc/mlm_mesh.h) built with g++ -fsanitize=address,undefined: the
  scratch bytes match the formula restated here over the box list of tests/test_cluster_plan.py, refused arguments are refused.  The
  contract refuses a box of more than 2^31 - 1 lattice points, which four boxes of that list are ((2^31 - 1, 1, 1) and
  (1290, 1290, 1290) among them: 1291^3 > 2^31 - 1): they are in the list here and must be refused.
* the rules of mlm_mesh.h (state byte, face mask, vertex predicate and normal sum, corner offsets, vertex position, numbering: the
  code the kernels run) driven phase by phase, sequentially, on class arrays generated here: all five arrays and the summary equal the
  numpy ground truth (tests/mesh_ref.py), which is itself checked for the three properties of a mesh.
* the binding's methods and constants."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
CHUNK, CTRL_BYTES = 2048, 256  # (mlm_mesh.h kMeshChunk, kMeshCtrlBytes)
I32 = 2 ** 31 - 1
SENT = 0x77

CLASS_FLAGS = [ref.OCC, ref.OCC | ref.INFL, ref.UNKNOWN, ref.OCC | ref.UNKNOWN]
FLAGS = [c | s | k for c in CLASS_FLAGS for s in (0, ref.SEEN) for k in (0, ref.CLOSED)]
BOXES = [(1, 1, 1), (67, 5, 7), (1, 200, 3), (64, 2, 1), (33, 9, 9)]  # (67 x 5 x 7: two chunks of 2048, x no multiple of 64)
SETS = ["full", "empty", "checkerboard", "random"]
GEOMETRY = [((-17, 3, 25), 10, 0.1), ((-2 ** 31, I32 - 200, -3), 7, 0.05), ((5, -403, 0), 3, 0.2)]  # lo, subbox_n, subbox_d_xyz


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("mp")
    exe = d / "mesh_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "mesh_driver.cpp"), "-o", str(exe)])

    def lines(mode, *cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(exe), mode, *args], check=True, capture_output=True, text=True).stdout
        return [[int(x) for x in line.split()] for line in out.splitlines()]

    def run(occ, infl, lo, flags, cap_f, cap_v, n, d_sub, which=31):
        gz, gy, gx = occ.shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([gx - 2, gy - 2, gz - 2, flags, cap_f, cap_v, *lo, n, which, 0], dtype=np.int64).tobytes())
            f.write(np.array([d_sub], dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(occ, dtype=np.int8).tobytes())
            f.write(np.ascontiguousarray(infl, dtype=np.int8).tobytes())
        subprocess.run([str(exe), "run", str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        out, at = {"summary": np.frombuffer(raw[:96], dtype=np.int64)}, 96
        for key, rows, cols, dt in (("quads", cap_f, 4, np.int32), ("faces", cap_f, 4, np.int32), ("verts", cap_v, 3, np.int32),
                                    ("xyz", cap_v, 3, np.float32), ("normals", cap_v, 3, np.int8)):
            size = rows * cols * np.dtype(dt).itemsize
            out[key] = np.frombuffer(raw[at:at + size], dtype=dt).reshape(rows, cols)
            at += size
        assert at == len(raw)
        return out

    return lines, run


def up(v):
    return (v + 255) // 256 * 256


# ---- the planner --------------------------------------------------------------------------------------------------------------
def test_plan_scratch(driver):
    lines, _ = driver
    boxes = [(1, 1, 1), (33, 9, 9), (32, 8, 8), (31, 7, 1), (1, 200, 3), (93, 73, 63), (512, 512, 64), (2 ** 31 - 1, 1, 1), (1, 1, 2 ** 31 - 1),
             (65536, 32767, 1), (1290, 1290, 1290)]  # (the list of tests/test_cluster_plan.py)
    boxes += [(2 ** 30, 1, 1), (1289, 1289, 1289), (I32 // 4 - 1, 1, 1), (I32 // 4, 1, 1), (67, 5, 7)]
    rows = lines("plan", *boxes)
    assert len(rows) == len(boxes)
    refused = 0
    for r, D in zip(rows, boxes):
        assert tuple(r[:3]) == D
        vox, lat, grown = D[0] * D[1] * D[2], (D[0] + 1) * (D[1] + 1) * (D[2] + 1), (D[0] + 2) * (D[1] + 2) * (D[2] + 2)
        if lat > I32:  # a vertex number would not fit an int32: refused although the voxels fit
            assert r[3] == 2 and vox <= I32, D
            refused += 1
            continue
        assert r[3] == 0, D
        words, fch, vch = (lat + 63) // 64, (vox + CHUNK - 1) // CHUNK, (lat + CHUNK - 1) // CHUNK
        assert r[4:10] == [vox, lat, grown, words, fch, vch]
        # per voxel a mask byte and (grown) a state byte, per 64 lattice points a u64 of bits and a u32 base, a u64 per chunk and one more
        parts = [up(grown), up(vox), up(8 * words), up(4 * words), up(8 * (fch + 1)), up(8 * (vch + 1))]
        assert r[10:16] == parts
        offs = np.cumsum(parts).tolist()
        assert r[16:22] == offs and r[22] == offs[-1] + CTRL_BYTES
    assert refused == 6 and rows[boxes.index((1289, 1289, 1289))][3] == 0 and rows[boxes.index((I32 // 4 - 1, 1, 1))][3] == 0


def test_plan_and_argument_refusals(driver):
    lines, _ = driver
    assert [r[3] for r in lines("plan", (0, 4, 4), (4, -1, 4), (4, 4, 0), (2 ** 31, 1, 1), (2 ** 30, 1, 1), (4, 4, 4))] == [1, 1, 1, 1, 2, 0]
    # flags, cap_faces, a face array given, cap_verts, a vertex array given, summary given
    good = [(1, 0, 0, 0, 0, 1), (7 | 16 | 32, 5, 1, 0, 0, 0), (2, 0, 0, 9, 1, 0), (4 | 32, 2 ** 40, 1, 2 ** 40, 1, 1), (1, 1, 1, 1, 1, 0)]
    assert [r[0] for r in lines("args", *good)] == [0] * len(good)
    bad = [((0, 0, 0, 0, 0, 1), 1), ((16, 0, 0, 0, 0, 1), 1), ((32 | 16, 0, 0, 0, 0, 1), 1), ((1 | 8, 0, 0, 0, 0, 1), 1), ((1 | 64, 0, 0, 0, 0, 1), 1),
           ((-1, 0, 0, 0, 0, 1), 1), ((1 | 1 << 30, 0, 0, 0, 0, 1), 1), ((1, -1, 1, 0, 0, 1), 2), ((1, 0, 0, -5, 1, 1), 2), ((1, 0, 1, 0, 0, 1), 3),
           ((1, 4, 0, 0, 0, 1), 3), ((1, 0, 0, 0, 1, 1), 3), ((1, 0, 0, 4, 0, 1), 3), ((1, 0, 0, 0, 0, 0), 4)]
    assert [r[0] for r in lines("args", *[b[0] for b in bad])] == [b[1] for b in bad]


def test_division_by_multiplication_is_exact(driver):
    lines, _ = driver
    bad, n = lines("div")[0]
    assert bad == 0 and n > 100000


# ---- the rules in the device's phase order ------------------------------------------------------------------------------------
COMBOS = [(o, i) for o in (0, 1, -1) for i in (0, -1)]  # (occ class, infl class)


def is_obstacle(flags, occ, infl):
    return bool((flags & ref.OCC and occ == 0) or (flags & ref.INFL and infl == 0) or (flags & ref.UNKNOWN and occ == -1))


def classes(kind, D, flags, rng):
    """class arrays of the grown box: voxels of the pattern draw a class pair the flags make an obstacle, the others one they do not"""
    shape = (D[2] + 2, D[1] + 2, D[0] + 2)
    if kind == "full":
        S = np.ones(shape, dtype=bool)
    elif kind == "empty":
        S = np.zeros(shape, dtype=bool)
    elif kind == "checkerboard":
        S = np.indices(shape).sum(axis=0) % 2 == 0
    else:
        S = rng.random(shape) < 0.4
    yes = np.array([c for c in COMBOS if is_obstacle(flags, *c)])
    no = np.array([c for c in COMBOS if not is_obstacle(flags, *c)])
    pick = np.where(S[..., None], yes[rng.integers(0, len(yes), size=shape)], no[rng.integers(0, len(no), size=shape)])
    return pick[..., 0].astype(np.int8), pick[..., 1].astype(np.int8)


def compare(got, exp, cap_f, cap_v, which, tag):
    F, V = int(exp["summary"][0]), int(exp["summary"][1])
    assert np.array_equal(got["summary"], exp["summary"]), (tag, got["summary"], exp["summary"])
    for bit, key, total, cap in ((1, "quads", F, cap_f), (2, "faces", F, cap_f), (4, "verts", V, cap_v), (8, "xyz", V, cap_v), (16, "normals", V, cap_v)):
        rows = min(total, cap) if which & bit else 0
        g = got[key]
        assert g[:rows].tobytes() == exp[key][:rows].tobytes(), (tag, key)
        assert (np.frombuffer(g[rows:].tobytes(), dtype=np.uint8) == SENT).all(), (tag, key, "rows beyond the cap were written")


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(map(str, b)))
def test_rules_against_numpy(driver, box):
    """every flag combination on every set; the four caps and a subset of the arrays on a rotating flag combination"""
    _, run = driver
    rng = np.random.default_rng(sum(box))
    turn = 0
    for kind in SETS:
        for fi, flags in enumerate(FLAGS):
            lo, n, d = GEOMETRY[(fi + turn) % len(GEOMETRY)]
            occ, infl = classes(kind, box, flags, rng)
            exp = ref.mesh(occ, infl, lo, flags, n, d)
            ref.check_properties(exp, flags)
            assert np.array_equal(ref.vertex_normals_from_faces(exp), exp["normals"])
            F, V = int(exp["summary"][0]), int(exp["summary"][1])
            tag = (box, kind, flags)
            if kind == "empty":
                assert F == 0 and V == 0
            if kind == "full" and flags & ref.CLOSED:  # the box itself: its six sides
                sides = [box[1] * box[2], box[0] * box[2], box[0] * box[1]]
                assert F == 2 * sum(sides) and list(exp["summary"][4:10]) == [s for s in sides for _ in (0, 1)] and exp["summary"][10] == F
            if kind == "full" and not flags & ref.CLOSED:
                assert F == 0  # (obstacles all around: nothing is open)
            compare(run(occ, infl, lo, flags, F + 1, V + 1, n, d), exp, F + 1, V + 1, 31, tag)
            if fi == (turn * 5) % len(FLAGS):
                for cap_f, cap_v in sorted({(0, 0), (max(F - 1, 0), max(V - 1, 0)), (F, V), (F + 1, V + 1), (0, V), (F, 0)}):
                    compare(run(occ, infl, lo, flags, cap_f, cap_v, n, d), exp, cap_f, cap_v, 31, tag + (cap_f, cap_v))
                compare(run(occ, infl, lo, flags, F + 1, V + 1, n, d, which=1 | 8), exp, F + 1, V + 1, 1 | 8, tag + ("quads and xyz only",))
        turn += 1


def test_reference_on_cases_known_by_hand():
    """a single voxel, and two voxels that touch at an edge: counted by hand"""
    occ = np.ones((3, 3, 3), dtype=np.int8)
    occ[1, 1, 1] = 0
    m = ref.mesh(occ, np.full(occ.shape, -1), (4, -9, 19), ref.OCC, 10, 0.1)
    assert list(m["summary"]) == [6, 8, 1, 1, 1, 1, 1, 1, 1, 1, 6, 0]
    assert np.array_equal(m["faces"], [[4, -9, 19, a] for a in range(6)])
    assert np.array_equal(m["verts"][0], [4, -9, 19]) and np.array_equal(m["verts"][-1], [5, -8, 20])
    assert np.array_equal(m["normals"][0], [-1, -1, -1]) and np.array_equal(m["normals"][-1], [1, 1, 1])
    assert m["xyz"].dtype == np.float32 and m["xyz"][0].tolist() == [np.float32(0.4), np.float32(-1.0 + 0.1), np.float32(1.0 + 9 * 0.1)]
    ref.check_properties(m, ref.OCC)
    occ = np.ones((3, 4, 4), dtype=np.int8)
    occ[1, 1, 1] = occ[1, 2, 2] = 0  # (0, 0, 0) and (1, 1, 0): they share the edge x = 1, y = 1
    m = ref.mesh(occ, np.full(occ.shape, -1), (0, 0, 0), ref.OCC | ref.CLOSED)
    assert m["summary"][0] == 12 and m["summary"][1] == 14 and m["summary"][10] == 8
    pinch = [i for i, k in enumerate(m["verts"].tolist()) if k[:2] == [1, 1]]
    assert len(pinch) == 2 and all(m["normals"][i, 0] == 0 and m["normals"][i, 1] == 0 for i in pinch)
    ref.check_properties(m, ref.OCC | ref.CLOSED)


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_binding_surface():
    from mlmapping_amd import mlmap

    assert (mlmap.MLM_MESH_OCC, mlmap.MLM_MESH_INFL, mlmap.MLM_MESH_UNKNOWN, mlmap.MLM_MESH_SEEN, mlmap.MLM_MESH_CLOSED) == (1, 2, 4, 16, 32)
    assert (ref.OCC, ref.INFL, ref.UNKNOWN, ref.SEEN, ref.CLOSED) == (1, 2, 4, 16, 32) and mlmap.MLM_MESH_ROW == ref.ROW == 12
    assert callable(mlmap.MLMap.export_mesh) and callable(mlmap.MLMap.export_mesh_dev)
    assert "mlm_export_mesh" in mlmap.ABI_SYMBOLS
    assert hasattr(mlmap.load_library(), "mlm_export_mesh")
    hdr = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    for name, v in (("OCC", "1"), ("INFL", "2"), ("UNKNOWN", "4"), ("SEEN", "16"), ("CLOSED", "32"), ("ROW", "12")):
        assert re.search(rf"#define MLM_MESH_{name} {v}(\s|$)", hdr), name
    assert re.search(r"#define MLM_ABI_VERSION 6(\s|$)", hdr)
    assert re.search(r"\bvoid exportMesh\(", open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read())
