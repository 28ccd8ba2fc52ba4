"""The read-outs' shared host arithmetic (mlmapping_amd/csrc/mlm_host.h), on the CPU: a stand-alone driver
(tests/cpp/readout_host_driver.cpp) built with g++ -fsanitize=address,undefined, its rows checked here.

* mlm_brick_cover against numpy.floor_divide, around zero and around the int32 edges;
* mlm_box_check's three answers, in the order the entry points report them;
* mlm_stage_layout for random subsets of the channels of the chunked queries: offsets, disjoint ranges, the closed formula;
* mlm_export_window's tiles: mlm_esdf_plan(D, H + 1, false, ...) gives what the window's own rule gave before it;
* mlm_for_tiles against the tile loops of window, esdf and grid2d as they were spelled out before it;
* mlm_stage_rows against the three lines of mlm_crop_blocks' page-out that it replaced.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _const(header, name):
    txt = open(os.path.join(CSRC, header)).read()
    return eval(re.search(rf"constexpr \w+(?: \w+)? {name} = ([^;]+);", txt).group(1).replace("ll", ""))


def _abi_define(name):
    txt = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    return int(re.search(rf"#define {name} (\d+)\b", txt).group(1))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ro") / "readout_host_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "readout_host_driver.cpp"), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
        return np.array([[int(x) for x in line.split()] for line in out.splitlines()], dtype=np.int64)

    return run


def test_brick_cover(driver):
    rows = driver("cover")
    n, lo, d, b0, nb = rows.T
    # the whole sweep is there: every brick edge, origins around zero and on both sides of the four int32 marks, every extent
    assert set(n) == {1, 2, 3, 4, 5, 8, 16}
    for e in (1, 2, 3, 4, 5, 8, 16):
        want_lo = set(range(-2 * e - 1, 2 * e + 2))
        for c in (I32_MIN - 64, I32_MIN, I32_MAX, I32_MAX + 64):
            want_lo |= set(range(c - 8, c + 9))
        assert set(lo[n == e]) == want_lo, e
        assert set(d[n == e]) == {v for v in (1, 2, e - 1, e, e + 1, 130) if v >= 1}, e
    assert len(np.unique(rows[:, :3], axis=0)) == sum(len(set(lo[n == e])) * len(set(d[n == e])) for e in (1, 2, 3, 4, 5, 8, 16))
    first, last = np.floor_divide(lo, n), np.floor_divide(lo + d - 1, n)
    assert np.array_equal(b0, first)
    assert np.array_equal(nb, last - first + 1)


def test_box_check(driver):
    top = 1 << 31
    cases = [
        # (lo, dims), rc
        (((0, 0, 0), (0, 1, 1)), 1), (((0, 0, 0), (1, 0, 1)), 1), (((0, 0, 0), (1, 1, 0)), 1),
        (((0, 0, 0), (-1, 1, 1)), 1), (((5, 5, 5), (1, -1, 1)), 1), (((0, 0, 0), (1, 1, -1)), 1),
        (((top - 2, 0, 0), (2, 1, 1)), 1),  # lo + dims = 2^31
        (((0, top - 5, 0), (1, 5, 1)), 1), (((0, 0, I32_MAX), (1, 1, 1)), 1),
        (((top - 3, 0, 0), (2, 1, 1)), 0),  # lo + dims = 2^31 - 1
        (((0, top - 6, 0), (1, 5, 1)), 0), (((0, 0, I32_MAX - 1), (1, 1, 1)), 0),
        (((0, 0, 0), (I32_MAX, 1, 1)), 0),
        (((0, 0, 0), (65536, 32768, 1)), 2),  # 2^31 voxels
        (((0, 0, 0), (65536, 32767, 1)), 0),
        (((I32_MIN, I32_MIN, I32_MIN), (2048, 1024, 1024)), 2),
        (((0, 0, 0), (0, 65536, 65536)), 1),  # wrong both ways: the first failure in axis order wins
        (((0, 0, 0), (65536, 65536, 0)), 2),
        (((-3, 4, I32_MIN), (7, 1, 9)), 0),
    ]
    rows = driver("box", *[v for (lo, dims), _ in cases for v in (*lo, *dims)])
    assert len(rows) == len(cases)
    for ((lo, dims), want), r in zip(cases, rows):
        assert r[0] == want, (lo, dims)
        if want == 0:  # D and nvox are the inputs
            assert tuple(r[1:4]) == dims and r[4] == dims[0] * dims[1] * dims[2], (lo, dims)


RENDER_ROW, BOX_ROW, PATH_ROW = _abi_define("MLM_RENDER_ROW"), _abi_define("MLM_BOX_ROW"), _abi_define("MLM_PATH_ROW")
# bytes per element of every channel, inputs first (the entry points' channel lists in mlmap_hip.hip)
RAYS = (24, 24, 1, 12, 8, 4, 4)
SWEEPS = RAYS + (12, 4)
RENDER = (96, 2, 1, 12, 4, RENDER_ROW * 8)
BOXES = (24, 1, 24, 1, BOX_ROW * 8)
NEAREST = (24, 1, 12, 12, 8, 8)


def paths_elems(cap):
    return (12, 1, cap * 12, 8, PATH_ROW * 8)


def align(b):
    return (b + 255) // 256 * 256


def layout_args(present, staged, elem, count):
    return [len(elem)] + [int(v) for c in range(len(elem)) for v in (present[c], staged[c], elem[c], count[c])]


def test_stage_layout(driver):
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(400):
        kind = rng.integers(4)
        if kind == 0:
            elem, count = RAYS, [int(rng.integers(1, 1 << 20))] * 7
        elif kind == 1:
            elem, count = SWEEPS, [int(rng.integers(1, 1 << 18))] * 9
        elif kind == 2:  # poses and table per pose, the rest per pixel of a chunk
            poses, pixels = int(rng.integers(1, 64)), int(rng.integers(1, 1 << 20))
            elem, count = RENDER, [poses, pixels, pixels, pixels, pixels, poses]
        else:
            elem, count = paths_elems(int(rng.integers(0, 300))), [int(rng.integers(1, 1 << 16))] * 5
        present = rng.random(len(elem)) < 0.7
        staged = rng.random(len(elem)) < 0.6  # (a staged flag on an absent channel must not count)
        cases.append((present, staged, elem, count))
    n_max = max(len(c[2]) for c in cases)
    assert n_max == 9
    # rows differ in length: one driver call per channel count
    for N in sorted({len(c[2]) for c in cases}):
        sub = [c for c in cases if len(c[2]) == N]
        rows = driver("layout", *[v for c in sub for v in layout_args(*c)])
        assert rows.shape == (len(sub), N + 1)
        for (present, staged, elem, count), r in zip(sub, rows):
            off, total = r[:N], r[N]
            takes = [align(count[c] * elem[c]) if present[c] and staged[c] else 0 for c in range(N)]
            assert total == sum(takes)  # the closed formula; absent and in-place channels take nothing
            assert (off % 256 == 0).all()
            assert list(off) == [sum(takes[:c]) for c in range(N)]  # ascending in channel order, ranges disjoint and packed
            for c in range(N):
                if takes[c]:
                    assert off[c] + count[c] * elem[c] <= (off[c + 1] if c + 1 < N else total)


def test_stage_layout_full_chunks(driver):
    """every channel staged, a full chunk: what tests of the chunk seams see in device_bytes"""
    box_chunk, near_chunk = _const("mlm_handle.h", "kBoxChunk"), _const("mlm_handle.h", "kNearChunk")
    assert (box_chunk, near_chunk) == (1 << 18, 1 << 18)
    r = driver("layout", *layout_args([1] * 5, [1] * 5, BOXES, [box_chunk] * 5))[0]
    assert r[-1] >= 82 * (1 << 18) and sum(BOXES) == 82
    r = driver("layout", *layout_args([1] * 6, [1] * 6, NEAREST, [near_chunk] * 6))[0]
    assert r[-1] >= 65 * (1 << 18) and sum(NEAREST) == 65


def test_for_tiles_is_the_loops_it_replaced(driver):
    """origins, extents and out_base of every tile, in order, against the transcribed z / y / x loops (and grid2d's y / x loops)"""
    cases = [  # dims of the walk, D, T
        (3, (1, 1, 1), (1, 1, 1)),
        (3, (5, 3, 2), (2, 2, 1)),
        (3, (5, 3, 2), (5, 3, 2)),  # a tile equal to the box
        (3, (5, 3, 2), (8, 4, 64)),  # a tile larger than the box
        (3, (7, 5, 3), (7, 2, 1)), (3, (7, 5, 3), (3, 1, 1)),  # mlm_esdf_plan's shapes: whole rows, a piece of a row
        (2, (5, 3, 1), (2, 2, 1)),  # a plane, as mlm_export_grid2d walks it
        (2, (9, 4, 1), (9, 3, 1)),
    ]
    rows = driver("tiles", *[v for nd, D, T in cases for v in (nd, *D, *T)])
    new, old = rows[rows[:, 0] == 0][:, 1:], rows[rows[:, 0] == 1][:, 1:]
    assert np.array_equal(new, old)
    for k, (nd, D, T) in enumerate(cases):
        t = new[new[:, 0] == k]
        n_tiles = int(np.prod([-(-d // s) for d, s in zip(D, T)]))
        assert len(t) == n_tiles, (D, T)
        org, td, base = t[:, 1:4], t[:, 4:7], t[:, 7]
        assert (td >= 1).all() and (org + td <= np.array(D)).all()
        assert td.prod(axis=1).sum() == np.prod(D)  # the tiles cover the box once
        assert np.array_equal(base, (org[:, 2] * D[1] + org[:, 1]) * D[0] + org[:, 0])
        assert list(map(tuple, org[:, ::-1])) == sorted(map(tuple, org[:, ::-1]))  # z outermost, x innermost
    assert driver("tiles_stop").tolist() == [[3, 7]]


def test_stage_rows_is_crop_runs_rule(driver):
    rows = driver("rows")
    n, per_row, cap, kv, got, before = rows.T
    wide = 12 + 6 * 512
    assert set(n) == {1, 2, 1000} and set(per_row) == {0, 1, 12, wide} and set(kv) == {0, 1, 6, 7, 1005}
    for p in (1, 12, wide):
        assert {1, p - 1, p, 64 << 20} <= set(cap[per_row == p])
    assert len(rows) == 3 * 4 * 4 * 3
    assert np.array_equal(got, before)
    assert ((got >= 1) & (got <= n)).all()
    assert (got[per_row == 0] == n[per_row == 0]).all()  # nothing staged: one round, whatever the knob
    staged = per_row > 0
    assert (got[staged & (kv > 0)] == np.minimum(n, kv)[staged & (kv > 0)]).all()
    free = staged & (kv == 0)
    assert (got[free] == np.minimum(n, np.maximum(1, cap // np.maximum(per_row, 1)))[free]).all()


def test_window_tiles_are_esdf_plan(driver):
    rows = driver("window")
    H, grad, staged = rows[:, 3], rows[:, 4], rows[:, 5]
    assert set(H) == set(range(9)) and set(grad) == {0, 1} and set(staged) == {0, 1}
    assert len(rows) > 5000
    plan_T, rule_T = rows[:, 6:9], rows[:, 9:12]
    assert np.array_equal(plan_T, rule_T)
    assert (plan_T >= 1).all()  # the planner's "no tile fits" answer does not occur
    assert np.array_equal(rows[:, 12], H)  # the planner's halo is the window's
    assert np.array_equal(rows[:, 13], np.prod(plan_T + 2 * H[:, None], axis=1))  # the haloed tile: the odds scratch
    D = rows[:, 0:3]
    assert (plan_T[:, 0] < D[:, 0]).any() and (plan_T[:, 1] < D[:, 1]).any() and (plan_T[:, 2] < D[:, 2]).any()  # every kind of cut
