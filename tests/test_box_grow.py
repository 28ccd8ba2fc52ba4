"""The box growth of mlm_query_boxes on the host (mlmapping_amd/csrc/mlm_boxgrow.h, the control flow the kernel runs too, under
MapView::boxes of mlm_mapview.h, which answers small batches from the library's host mirror), built for the CPU with
-fsanitize=address,undefined and held to the contract written in plain Python integers (tests/box_ref.py) over the oracle's voxel
classes: every output of every flag set.  The Python reference itself is held to properties first."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1, SDEF
from tests import box_ref as br
from tests import raywalk_ref as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_map(rng, n, nblk=40, span=3, p_occ=0.02, p_unk=0.05, p_infl=0.03, released=0.15):
    """a block dump of random classes: blocks of a (2 span)^3 lattice of block indices around 0, some absent, some released"""
    keys = np.unique(rng.integers(-span, span, size=(nblk, 3)), axis=0).astype(np.int32)
    c = n ** 3
    r = rng.random((len(keys), c))
    occ = np.where(r < p_occ, ord("o"), np.where(r < p_occ + p_unk, ord("u"), ord("f"))).astype(np.uint8)
    infl = np.where(rng.random((len(keys), c)) < p_infl, ord("o"), ord("u")).astype(np.uint8)
    col = (rng.random(len(keys)) < released).astype(np.uint8)
    occ[col.astype(bool), 0] = rng.choice([ord("f"), ord("f"), ord("u"), ord("o")], size=int(col.sum()))
    return {"keys": keys, "occ": occ, "infl": infl, "collapsed": col}


def random_boxes(rng, lo, hi, count, side=4):
    a = rng.integers(lo, hi, size=(count, 3))
    b = a + rng.integers(0, side, size=(count, 3)) * (rng.random((count, 3)) < 0.6)
    return np.concatenate([a, b], axis=1).astype(np.int32)


WEIRD = np.array([[3, 0, 0, 2, 0, 0],                                  # a > b
                  [0, 0, 5, 0, 0, 4],
                  [0, 0, 0, 2 ** 15, 0, 0],                            # a side of 2^15 + 1
                  [br.I32_MIN, 0, 0, br.I32_MIN + 1, 0, 0],            # at the int32 edges: absent space, closed by limit, no wrap
                  [0, br.I32_MAX, 0, 0, br.I32_MAX, 0],
                  [br.I32_MIN, br.I32_MIN, br.I32_MIN, br.I32_MIN, br.I32_MIN, br.I32_MIN],
                  [br.I32_MAX - 2, br.I32_MAX - 1, br.I32_MAX, br.I32_MAX - 1, br.I32_MAX, br.I32_MAX],
                  [5000000, 0, 0, 5000003, 0, 0]], dtype=np.int64).astype(np.int32)  # far from the map, inside the key range


def test_python_growth_has_the_properties():
    """on random maps, for every flag set, random max_grow and windows: B0 inside the result, no O voxel in it, within the limits, an
    O voxel in the adjacent slab of every face closed by obstacle, every other face exactly at a limit"""
    rng = np.random.default_rng(3)
    seen = {-1: 0, 0: 0, 1: 0}
    by_obstacle = by_limit = 0
    for trial in range(9):
        n = [5, 4, 7][trial % 3]
        classes = rw.block_classes(random_map(rng, n), n)
        boxes = np.concatenate([random_boxes(rng, -3 * n - 2, 3 * n + 2, 40), WEIRD])
        for f in br.FLAG_SETS:
            mg = [int(v) for v in rng.integers(0, 7, size=6)] if trial % 2 else [int(rng.integers(0, 9))] * 6
            wlo = [int(v) for v in rng.integers(-3 * n - 1, -2 * n, size=3)]
            window = None if (trial + f) % 3 == 0 else (wlo, [int(v) for v in rng.integers(4 * n, 7 * n, size=3)])
            for b in boxes:
                res = br.grow(b, f, classes, mg, window)
                seen[br.check_properties(b, f, classes, mg, window, res)] += 1
                if res[0] == 1:
                    by_obstacle += bin(res[2]).count("1")
                    by_limit += 6 - bin(res[2]).count("1")
    assert min(seen.values()) >= 100 and by_obstacle >= 500 and by_limit >= 500, (seen, by_obstacle, by_limit)
    # the contract's example of order dependence: the only obstacle at (-1,-1,0); -x absorbs (-1,0,0) first, then -y is closed by it
    only = lambda v: np.where((np.asarray(v) == [-1, -1, 0]).all(axis=1), br.OCC, 0)
    assert br.grow([0, 0, 0, 0, 0, 0], br.OCC, only, [3] * 6) == (1, (-3, 0, -3, 3, 3, 3), 1 << 2, (7 * 4 * 7, 0, 0, 3 + 3 + 3 + 3 + 3))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("boxes") / "box_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "box_driver.cpp"), "-o", str(out)])
    return str(out)


def run_driver(exe, path, d_sub, n, b, boxes, cases):
    """cases: [(flags, max_grow[6] or None, window or None)] -> [{"status", "box", "closed", "table"}]"""
    rows = []
    for f, mg, w in cases:
        rows.append([f, 0 if w is None else 1] + ([0] * 6 if mg is None else list(mg)) + ([0] * 6 if w is None else list(w[0]) + list(w[1])))
    blob = struct.pack("<d4i", d_sub, n, b["keys"].shape[0], len(boxes), len(cases))
    blob += np.array(rows, dtype=np.int32).tobytes()
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    blob += np.ascontiguousarray(boxes, dtype=np.int32).tobytes()
    path.write_bytes(blob)
    out = [ln.split() for ln in subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    m = len(boxes)
    assert len(out) == m * len(cases)
    res = []
    for k in range(len(cases)):
        r = np.array([[int(x) for x in row] for row in out[k * m:(k + 1) * m]], dtype=np.int64).reshape(m, 12)
        res.append({"status": r[:, 0].astype(np.int8), "box": r[:, 1:7].astype(np.int32), "closed": r[:, 7].astype(np.uint8), "table": r[:, 8:12].copy()})
    return res


def hold(exe, path, d_sub, n, b, boxes, cases, what, min_grown=1):
    classes = rw.block_classes(b, n)
    got = run_driver(exe, path, d_sub, n, b, boxes, cases)
    grown = 0
    for (f, mg, w), g in zip(cases, got):
        exp = br.grow_all(boxes, f, classes, mg, w)
        br.assert_equal(g, exp, f"{what} flags={f} max_grow={mg} window={w}")
        grown += int(exp["table"][:, 3].sum())
    assert grown >= min_grown, grown
    return got


def test_host_boxes_equal_the_reference_on_crafted_maps(exe, tmp_path):
    rng = np.random.default_rng(8)
    for trial, n in enumerate((5, 4, 10)):
        b = random_map(rng, n, p_occ=0.01 if n == 10 else 0.02)
        boxes = np.concatenate([random_boxes(rng, -3 * n - 2, 3 * n + 2, 60), WEIRD])
        cases = []
        for f in br.FLAG_SETS:
            cases.append((f, [int(v) for v in rng.integers(0, 6, size=6)], None))
            cases.append((f, [4] * 6, ([-2 * n - 1, -2 * n, -n - 2], [4 * n, 3 * n + 1, 3 * n])))
        cases.append((br.OCC, None, None))  # a pure count
        hold(exe, tmp_path / f"crafted{trial}.bin", 0.2, n, b, boxes, cases, f"crafted n={n}", min_grown=500)


@pytest.mark.parametrize("name", ["SDEF", "S1 frontier n5 (released blocks)"])
def test_host_boxes_equal_the_reference_on_oracle_maps(exe, tmp_path, name):
    from oracle.binding import OracleMap

    released = "released" in name
    cfg = SDEF.with_(depth_noise_coe=0.00375, lm_occupied_sh=2.0) if not released else S1.with_(use_exploration_frontiers=True, subbox_n=5)
    cpu = OracleMap(cfg)
    shift = np.array([-8.0, -7.5, 0.0])
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 4):
        cpu.update_depth(img, q, np.array(t) + shift)  # (a map in negative x, y; frontier bookkeeping and inflation need z in [0, 5))
    b = cpu.export_blocks()
    full = (b["occ"] == ord("o")).any(axis=1) & ~b["collapsed"].astype(bool)
    cpu.inflate_map((np.median(b["keys"][full], axis=0) + 0.5) * cfg.subbox_d_xyz * cfg.subbox_n)
    b = cpu.export_blocks()
    if released:
        assert b["collapsed"].any()
    n = cfg.subbox_n
    rng = np.random.default_rng(13)
    lo, hi = b["keys"].min(0) * n - 3, (b["keys"].max(0) + 1) * n + 3
    # seeds: FREE voxels (the boxes that grow), and boxes anywhere
    vox = rng.integers(lo, hi, size=(40000, 3))
    free = vox[rw.block_classes(b, n)(vox) == 0][:80]
    assert len(free) == 80
    boxes = np.concatenate([np.concatenate([free, free], axis=1).astype(np.int32), random_boxes(rng, lo, hi, 60), WEIRD])
    cases = [(f, [6] * 6, None) for f in br.FLAG_SETS] + [(br.OCC | br.UNKNOWN, [3, 9, 0, 2, 12, 1], ([int(v) for v in lo + 5], [int(v) for v in (hi - lo) - 9])),
                                                         (br.OCC | br.INFL, None, None)]
    got = hold(exe, tmp_path / "oracle.bin", cfg.subbox_d_xyz, n, b, boxes, cases, name, min_grown=2000)
    assert len({int(c) for g in got for c in g["closed"]}) >= 8  # (faces closed by obstacle in many combinations)
