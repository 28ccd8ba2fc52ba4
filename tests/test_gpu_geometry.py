"""The map under launch geometries far from the tuned defaults, CU masks, and the FP64 fall-back of the hit increment.

The kernels spread their work with grid-stride loops, per-wave strides and counter draws; at the default geometry a frame's work is
often done in one turn and the code of the later turns never runs.  One fixed workload — an 8-frame batch (the n > 4 grids), a
3-frame batch, single frames through the graph, sparse pixel lists followed by a dense frame alone and in a batch (the adaptive chain
grid at its minimum) — runs in the default mode and in frontier mode under every setting of SETTINGS, and after every step the map
(float bits), the awareness lists, the frontier set and the queries at voxel centres must be the oracle's.  The oracle's states are
computed once (they do not depend on the knobs).  Nothing here launches a knob value mlm_debug_set refuses (tests/test_abi.py)."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1, SDEF
from tests.util import GRID_KNOBS, ODDS_TOL, compare_maps, odds_of, voxel_centres

pytestmark = pytest.mark.gpu

MODES = {"default": S1, "frontier": S1.with_(use_exploration_frontiers=True, subbox_n=5)}
SPARSE_N = 1500  # pixels of a sparse pixel-list frame


def _grids(f):
    return {k: f(k, d) for k, d in GRID_KNOBS.items()}


ODD = (3, 7, 13)
CELL_TABLE_MIN = {"collect_grid": 1, "sort_grid": 1, "expand_block": 64, "sort_block": 64, "sc_block": 64}
CELL_TABLE_MAX = {"collect_grid": 4096, "sort_grid": 4096, "expand_block": 256, "sort_block": 256, "sc_block": 256}
FAIL_2 = {"sec_fail_every": 2, "sec_backoff": 0}  # every 2nd frame's Stage A overflows on purpose and is redone on the cell-table path
# (id, knobs, modes): every entry pairs its knobs with what makes their kernels run
SETTINGS = [
    ("defaults", {}, ("default", "frontier")),
    ("grids_1", _grids(lambda k, d: 1), ("default", "frontier")),
    ("grids_1_cell_table_every_2nd", {**_grids(lambda k, d: 1), **FAIL_2}, ("default", "frontier")),
    ("grids_3_7_13", _grids(lambda k, d: ODD[sorted(GRID_KNOBS).index(k) % 3]), ("default", "frontier")),
    ("grids_7_13_3", {**_grids(lambda k, d: ODD[(sorted(GRID_KNOBS).index(k) + 1) % 3]), **FAIL_2}, ("default", "frontier")),
    ("grids_13_3_7", _grids(lambda k, d: ODD[(sorted(GRID_KNOBS).index(k) + 2) % 3]), ("default", "frontier")),
    # 2-4x the defaults; chain_grid (adaptive, 8 .. 128) at 256, tile_grid at n_tiles (mlm_create clamps it there)
    ("grids_2x_4x", {**_grids(lambda k, d: (2 + sorted(GRID_KNOBS).index(k) % 3) * d), "chain_grid": 256, "tile_grid": 1 << 20},
     ("default", "frontier")),
    ("cell_table_min", {**CELL_TABLE_MIN, "sectors": 0}, ("default", "frontier")),
    ("cell_table_max", {**CELL_TABLE_MAX, "sectors": 0}, ("default", "frontier")),
    ("cell_table_192", {"expand_block": 192, "sort_block": 192, "sc_block": 192, "collect_grid": 3, "sort_grid": 7, "sectors": 0},
     ("default", "frontier")),
    ("cell_table_min_every_2nd", {**CELL_TABLE_MIN, **FAIL_2}, ("default", "frontier")),
    ("cell_table_max_every_2nd", {**CELL_TABLE_MAX, **FAIL_2}, ("default", "frontier")),
    ("single_apply_grid_1", {"single_apply_grid": 1}, ("default",)),  # (k_apply_single: a dense frame's records in many turns)
    ("single_apply_grid_2", {"single_apply_grid": 2}, ("default",)),
    ("bin_block_512", {"bin_block": 512}, ("default", "frontier")),
    ("bin_block_1024", {"bin_block": 1024}, ("default", "frontier")),
    ("cu_split_8", {"cu_split": 8}, ("default", "frontier")),
    ("cu_reserve_16", {"cu_reserve": 16}, ("default", "frontier")),
    ("cu_split_8_reserve_16", {"cu_split": 8, "cu_reserve": 16}, ("default", "frontier")),
]


def _workload(cfg):
    """[(step name, [(kind, image, pose index, pixel list or None)])]: what both maps integrate, step by step."""
    frames = [img for img, _ in syn.stream(cfg, "room_jitter", "random", 8, seed=11)]
    poses = syn.random_poses(26, seed=17)
    rng = np.random.default_rng(5)
    nxt = iter(range(len(poses)))

    def dense(i):
        return ("dense", frames[i], poses[next(nxt)], None)

    def sparse(i):
        return ("sparse", frames[i], poses[next(nxt)], rng.choice(frames[i].size, SPARSE_N, replace=False).astype(np.int32))

    return [
        ("batch of 8", [dense(i) for i in range(8)]),
        ("batch of 3", [dense(i) for i in (1, 3, 5)]),
        ("single frame 1", [dense(2)]),
        ("single frame 2", [dense(6)]),
        ("sparse pixel lists", [sparse(i) for i in (0, 4, 7)]),
        ("dense frame alone after sparse ones", [dense(3)]),
        ("sparse pixel lists again", [sparse(i) for i in (1, 2, 6)]),
        ("batch of 5 after sparse frames", [dense(i) for i in (7, 0, 5, 2, 4)]),
    ]


def _run_step(m, step, is_oracle):
    name, items = step
    if is_oracle:
        for kind, img, (q, t), pix in items:
            if kind == "sparse":
                m.update_depth_indexed(img, pix, q, t)
            else:
                m.update_depth(img, q, t)
        return
    if name.startswith("batch"):
        m.update_map_batch(np.stack([it[1] for it in items]), np.stack([it[2][0] for it in items]), np.stack([it[2][1] for it in items]))
    elif name.startswith("dense frame alone"):
        # (submitted asynchronously: the general single-frame submission, whose k_chain_lanes grid adapts to the last frame's cells —
        # a sparse frame's few leave it at its minimum for this dense one; the graph's grid is single_chain_grid)
        m.set_async(True)
        _, img, (q, t), _ = items[0]
        m.update_map(img, q, t)
        m.sync()
        m.set_async(False)
    else:
        for kind, img, (q, t), pix in items:
            m.update_map(img, q, t, pixel_idx=pix)


def _snapshot(cpu, cfg):
    b = cpu.export_blocks()
    cells, odds = cpu.hit_cells_sorted()
    pos = voxel_centres(b, cfg, limit=20000)
    return {"blocks": b, "hit_cells": cells, "hit_odds": odds, "misses": np.sort(cpu.misses()).astype(np.int64),
            "n_oor": cpu.out_of_range_count(), "bkt": cpu.hit_bucket_count(),
            "frontier": cpu.export_frontier() if cfg.use_exploration_frontiers else None,
            "pos": pos, "occ": cpu.getOccupancy(pos), "odd": cpu.getOdd(pos)}


@pytest.fixture(scope="module")
def oracle_states():
    """{mode: (workload, [oracle state after each step])}"""
    from oracle.binding import OracleMap

    out = {}
    for mode, cfg in MODES.items():
        steps = _workload(cfg)
        cpu, snaps = OracleMap(cfg), []
        for step in steps:
            _run_step(cpu, step, True)
            snaps.append(_snapshot(cpu, cfg))
        out[mode] = (steps, snaps)
    return out


def _check(gpu, s, what):
    """the GPU map against one oracle state: _awareness_equal of tests/test_gpu_parity.py, the block dump bit for bit, the frontier
    set, and the queries at (a sample of) the voxel centres"""
    gc, go, _ = gpu.awareness_hits()
    assert np.array_equal(gc, s["hit_cells"]), f"{what}: hit cell sets differ"
    assert np.array_equal(go.view(np.uint32), s["hit_odds"].view(np.uint32)), f"{what}: hit odds differ (float bits)"
    assert np.array_equal(gpu.awareness_misses(), s["misses"]), f"{what}: miss cell sets differ"
    st = gpu.frame_stats()
    assert st["n_out_of_range"] == s["n_oor"], f"{what}: out-of-range points"
    assert st["hit_bucket_count"] == s["bkt"], f"{what}: hit container bucket count"
    compare_maps(gpu.export_blocks(), s["blocks"], what)
    if s["frontier"] is not None:
        assert np.array_equal(gpu.export_frontier(), s["frontier"]), f"{what}: frontier sets differ"
    assert np.array_equal(gpu.getOccupancy(s["pos"]), s["occ"]), f"{what}: getOccupancy at voxel centres"
    d = np.abs(gpu.getOdd(s["pos"]).astype(np.float64) - s["odd"])
    assert d.max() <= 1e-6, f"{what}: getOdd at voxel centres, max difference {d.max():.3e}"


@pytest.mark.parametrize("setting,kn,modes", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_launch_geometry(oracle_states, knobs, setting, kn, modes):
    from mlmapping_amd import mlmap
    from mlmapping_amd.mlmap import MLMap

    for mode in modes:
        steps, snaps = oracle_states[mode]
        for name, v in kn.items():
            knobs.set(name, v)
        gpu = MLMap(MODES[mode], max_blocks=8192, max_batch=8, record_awareness=True)
        mlmap.debug_reset()  # (read by mlm_create)
        try:
            for k, (step, s) in enumerate(zip(steps, snaps)):
                what = f"setting {setting} {kn}, {mode} mode, step {k} ({step[0]})"
                try:
                    _run_step(gpu, step, False)
                except mlmap.MlmError as e:
                    raise AssertionError(f"{what}: {e}") from e
                _check(gpu, s, what)
            st = gpu.frame_stats()
            off_sectors = kn.get("sectors") == 0 or "bin_block" in kn  # (k_bin_points' 512 / 1024 tiles exist on the cell-table path only)
            if off_sectors:  # the cell-table path throughout: nothing falls back, no single frame takes the sector path's graph
                assert st["n_sector_fallbacks"] == 0 and st["n_graph_launches"] == 0, (setting, mode, st)
            elif "sec_fail_every" in kn:
                assert st["n_sector_fallbacks"] >= 5, (setting, mode, st)
            elif mode == "default":  # (the sector path, its single frames through the graph)
                assert st["n_sector_fallbacks"] == 0 and st["n_graph_launches"] >= 5, (setting, mode, st)
        finally:
            gpu.close()


@pytest.mark.parametrize("big_grid", [1, 3])
def test_large_table_pass_grid(knobs, monkeypatch, capfd, big_grid):
    """k_sector_big (the columns that overflowed their LDS cell table, drawn from a counter by big_grid workgroups) on the noisy scene
    of tests/test_gpu_parity.py::test_column_table_widens_with_the_scene, whose columns overflow the table S1 starts with (512
    entries: a smaller one would take S1 off the sector path, its miss bitmap no longer fits).  As there: the map equals the oracle's
    in single frames and in batches, and the table is widened — the large-table pass ran rather than frames falling back."""
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    monkeypatch.setenv("MLM_DEBUG_CREATE", "1")
    knobs.set("big_grid", big_grid)
    cfg = S1
    base = syn.room_depth(cfg)
    frames = np.stack([syn.jitter_depth(base, k, amp_mm=3000, seed=3) for k in range(4)])
    poses = syn.random_poses(12, seed=3)
    q = np.stack([p[0] for p in poses])
    t = np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_batch=4), OracleMap(cfg)
    for k in range(4):
        gpu.update_map(frames[k], q[k], t[k])
        cpu.update_depth(frames[k], q[k], t[k])
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"big_grid {big_grid}: noisy scene, single frame {k}")
    for k0 in (4, 8):
        gpu.update_map_batch(frames, q[k0:k0 + 4], t[k0:k0 + 4])
        for j in range(4):
            cpu.update_depth(frames[j], q[k0 + j], t[k0 + j])
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"big_grid {big_grid}: noisy scene, batch from frame {k0}")
    st = gpu.frame_stats()
    gpu.close()
    err = capfd.readouterr().err
    assert "cell table widened" in err, err[-2000:]
    assert st["n_sector_fallbacks"] <= 2, st


def test_create_lines_equal_the_recorded_ones(knobs, monkeypatch, capfd):
    """Three cases of tests/golden/create_plan.json (what mlm_create arrived at before its arithmetic became mlm_plan.h: see
    tests/test_create_plan.py) on the device: both MLM_DEBUG_CREATE lines byte for byte — the path, LDS bytes, table entries, grid
    and tiles, and through the device-memory total every capacity of the frame slots — and one frame against the oracle."""
    import json
    import os

    from mlmapping_amd import mlmap
    from mlmapping_amd.config import CONFIG2_YAML, CConfig, to_c
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_plan.json")))["cases"]
    monkeypatch.setenv("MLM_DEBUG_CREATE", "1")
    for name, cfg in (("S1", S1), ("frontier", CONFIG2_YAML), ("knob_sectors_0", S1)):
        case = next(c for c in golden if c["name"] == name)
        c_cfg, lim = to_c(cfg), case["lim"]
        for field, _ in CConfig._fields_:  # (the preset is the recorded configuration)
            v = getattr(c_cfg, field)
            assert (list(v) if field == "T_bs" else v) == case["cfg"][field], (name, field)
        assert (lim["max_blocks"], lim["max_batch"], lim["record_awareness"]) == (1024, 2, 0)
        for k, v in case["knobs"].items():
            knobs.set(k, v)
        capfd.readouterr()
        gpu, cpu = MLMap(cfg, max_blocks=lim["max_blocks"], max_points=lim["max_points"], max_batch=lim["max_batch"]), OracleMap(cfg)
        mlmap.debug_reset()
        lines = [ln + "\n" for ln in capfd.readouterr().err.splitlines() if ln.startswith("[create]")]
        assert lines == [case["line1"], case["line2"]], (name, lines)
        img = syn.room_depth(cfg)
        q, t = syn.translating_pose(1)
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
        assert compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"recorded case {name}, one frame")["bit_mismatch"] == 0
        gpu.close()


def test_cu_reserve_that_leaves_stage_a_no_cu_is_refused(knobs):
    """cu_reserve (or cu_split) equal to the CU count would give Stage A's streams an empty CU mask: mlm_create refuses it, and the
    next handle, made with the default knobs, works.  One CU left is accepted and gives the oracle's map."""
    import torch

    from mlmapping_amd import mlmap
    from mlmapping_amd.mlmap import MLMap, MlmError
    from oracle.binding import OracleMap

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert ncu > 16
    cfg = SDEF
    img = syn.room_depth(cfg)
    for name, v in (("cu_reserve", ncu), ("cu_split", ncu), ("cu_reserve", ncu + 5)):
        knobs.set(name, v)
        with pytest.raises(MlmError, match="INVALID"):
            MLMap(cfg, max_blocks=2048, max_batch=2)
        mlmap.debug_reset()
    for kn in ({}, {"cu_reserve": ncu - 1}):
        for name, v in kn.items():
            knobs.set(name, v)
        gpu, cpu = MLMap(cfg, max_blocks=2048, max_batch=2), OracleMap(cfg)
        mlmap.debug_reset()
        for k in range(2):
            q, t = syn.translating_pose(k)
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"after the refused handles, knobs {kn}")
        gpu.close()


def _libm_log10f():
    libm = ctypes.CDLL("libm.so.6")
    f = libm.log10f
    f.argtypes, f.restype = [ctypes.c_float], ctypes.c_float
    return f


def test_log10_fallback_against_fp64(knobs):
    """knob logit_exact = 0 takes the path of a host whose log10f is not the glibc one mlm_glibc_log10f restates: every hit increment
    is log10(odd / (1 - odd)) in FP64, rounded to float once (mlm_logit).  On a fresh map and a frame of hits only (no ray casting,
    scattered pixels), every voxel whose oracle log-odds is exactly one table increment — host log10f of entry r = float(p) / float(1 - p) — must hold float(log10(double(r)))
    of that entry; then a stream agrees with the oracle within ODDS_TOL, its occupancy classes except within the accumulated error of
    one increment's rounding per increment from the threshold."""
    from mlmapping_amd import mlmap
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    log10f = _libm_log10f()
    cfg = S1.with_(use_raycasting=False)
    img = syn.room_depth(cfg)
    q, t = syn.static_pose()
    gpu = MLMap(cfg, max_blocks=4096)
    gpu.update_map(img, q, t)
    assert gpu.frame_stats()["logit_bit_exact"] == 1
    gpu.close()
    # the increments of the table's entries: host log10f (what the oracle adds) and FP64 log10 rounded once (what the GPU must add)
    p = OracleMap(cfg).odds_table().ravel().astype(np.float32)
    p = p[(p > 0) & (p < 1)]
    r = p / (np.float32(1) - p)
    assert r.dtype == np.float32
    host = np.array([log10f(float(x)) for x in r], dtype=np.float32)
    fp64 = np.log10(r.astype(np.float64)).astype(np.float32)
    by_host = {}
    for hb, v in zip(host.view(np.uint32), fp64.view(np.uint32)):
        by_host.setdefault(int(hb), set()).add(int(v))
    host_bits = np.array(sorted(by_host), dtype=np.uint32)
    # a dense frame leaves no voxel with a single hit (the cells of neighbouring pixels share voxels): scattered pixels do — 4 000 of
    # them (a small frame: k_rank runs the chains) and 8 000 (k_chain_lanes)
    for n_pix in (4000, 8000):
        knobs.set("logit_exact", 0)
        gpu, cpu = MLMap(cfg, max_blocks=4096), OracleMap(cfg)
        mlmap.debug_reset()
        pix = np.random.default_rng(n_pix).choice(img.size, n_pix, replace=False).astype(np.int32)
        gpu.update_map(img, q, t, pixel_idx=pix)
        cpu.update_depth_indexed(img, pix, q, t)
        assert gpu.frame_stats()["logit_bit_exact"] == 0
        g, c = gpu.export_blocks(), cpu.export_blocks()
        gpu.close()
        assert np.array_equal(g["keys"], c["keys"])
        lo_c, lo_g = c["log_odds"].ravel().view(np.uint32), g["log_odds"].ravel().view(np.uint32)
        one = np.flatnonzero(np.isin(lo_c, host_bits))
        for i in one:
            want = by_host[int(lo_c[i])]
            assert int(lo_g[i]) in want, (f"{n_pix} pixels, voxel {i}: oracle {lo_c[i:i + 1].view(np.float32)[0]!r}, GPU "
                                          f"{lo_g[i:i + 1].view(np.float32)[0]!r}, FP64 increment(s) {np.array(sorted(want), np.uint32).view(np.float32)}")
        differ = int((lo_g[one] != lo_c[one]).sum())
        assert one.size >= 1000, one.size
        print(f"log10 fall-back, {n_pix} pixels: {one.size} single-increment voxels checked, {differ} differ from the host log10f in the last place")

    # a normal stream (ray casting on) under the fall-back
    cfg = S1
    knobs.set("logit_exact", 0)
    gpu, cpu = MLMap(cfg, max_blocks=8192, max_batch=4), OracleMap(cfg)
    mlmap.debug_reset()
    frames = list(syn.stream(cfg, "room_jitter", "random", 8, seed=9))
    for k, (img, (q, t)) in enumerate(frames):
        if k < 4:
            gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    gpu.update_map_batch(np.stack([f[0] for f in frames[4:]]), np.stack([f[1][0] for f in frames[4:]]), np.stack([f[1][1] for f in frames[4:]]))
    assert gpu.frame_stats()["logit_bit_exact"] == 0
    g, c = gpu.export_blocks(), cpu.export_blocks()
    assert np.array_equal(g["keys"], c["keys"]) and np.array_equal(g["collapsed"], c["collapsed"])
    dodd = np.abs(odds_of(g["log_odds"]) - odds_of(c["log_odds"]))
    assert dodd.max() <= ODDS_TOL, dodd.max()
    # a voxel takes at most one increment per awareness cell centre inside it per frame (a hit or a miss, each rounded differently at
    # most once by one last place of the largest |log-odds|, and its addition once more)
    cells_per_voxel = (np.ceil(cfg.subbox_d_xyz / cfg.am_d_Rho) + 2) * (np.ceil(cfg.subbox_d_xyz / cfg.am_d_Z) + 2) * cfg.n_phi
    ulp = float(np.spacing(np.float32(max(abs(cfg.lm_log_odds_min), abs(cfg.lm_log_odds_max)))))
    bound = len(frames) * cells_per_voxel * 2 * ulp
    bad = g["occ"] != c["occ"]
    near = np.abs(c["log_odds"].astype(np.float64) - cfg.lm_occupied_sh) <= bound
    assert not (bad & ~near).any(), f"{int((bad & ~near).sum())} voxels differ in occupancy class away from the threshold (bound {bound:.2e})"
    print(f"log10 fall-back stream: max |d odd| {dodd.max():.2e}, bit differences {int((g['log_odds'] != c['log_odds']).sum())}, "
          f"classes differing near the threshold {int(bad.sum())}")
    gpu.close()
