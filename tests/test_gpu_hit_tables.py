"""Order-free hit values from the handle's tables (MlmDev::hit_p / hit_inc / logit_one, k_fill_hit_tables; k_sector's hit-list phase):
a cell that receives n contributions of ONE kind ends at p_n = n applications of p <- 1 - (1 - p)(1 - a) (update_odds_hashmap,
map_awareness.h:147-154) and adds logit(p_n) (map_local.h:8, map_local.cpp:159).  Point-list frames of n copies of one point give such
cells with exactly n contributions — the centre cell (kind 0) and every spread neighbour (kinds 1 .. 20) —, so the frames below sit on
both sides of the table's end: n <= N is one load, n > N continues the chain from the table's last entry; N = 4 (knob hit_tab_n), the
default 256, and no table at all (0: the loop as it was).  rho at index 1 (kind-0 odd >= 0.5: the chain saturates at 1.0f), mid-range
and nRho - 2 (small odds: the chain's fixed point is 1 - 2^-24, it never leaves early).  Hit odds (float bits, record_awareness) and
the map's log-odds (float bits) against the oracle."""
import math

import numpy as np
import pytest

from mlmapping_amd.config import S1
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

IDENT = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)


def _point(cfg, rho_idx, theta, z_b=0.03):
    """sensor-frame point whose body-frame position is (r cos theta, r sin theta, z_b), r the centre of range step rho_idx
    (T_B_S of the presets: x_b = z_s + 0.12, y_b = -x_s, z_b = -y_s; identity pose: the awareness frame is the body's)"""
    r = (rho_idx + 0.5) * cfg.am_d_Rho
    xb, yb = r * math.cos(theta), r * math.sin(theta)
    return np.array([-yb, -z_b, xb - 0.12])


def _frame(cfg, n, k):
    """n copies each of three points, at rho index 1, mid-range and nRho - 2, in the k-th azimuth (frames do not share cells)"""
    theta = math.radians(7.3 + 23.0 * k)
    pts = [_point(cfg, r, theta + 0.2 * j) for j, r in enumerate((1, cfg.am_n_Rho // 2, cfg.am_n_Rho - 2))]
    return np.repeat(np.array(pts), n, axis=0)


def _check_hits(gpu, cpu, what):
    gc, go, _ = gpu.awareness_hits()
    cc, co = cpu.hit_cells_sorted()
    assert np.array_equal(gc, cc), f"{what}: hit cells differ"
    assert np.array_equal(go.view(np.uint32), co.view(np.uint32)), f"{what}: hit odds differ in bits"


CASES = [(4, (1, 3, 4, 5, 40)), (None, (255, 256, 257, 700)), (0, (1, 5, 40, 257))]


@pytest.mark.parametrize("record", [True, False], ids=["record_awareness", "no_record"])
@pytest.mark.parametrize("tab_n,counts", CASES, ids=["tab4", "default", "tab0"])
def test_single_kind_cells_on_both_sides_of_the_table_end(knobs, tab_n, counts, record):
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    cfg = S1
    if tab_n is not None:
        knobs.set("hit_tab_n", tab_n)
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_points=4096, record_awareness=record, max_batch=2), OracleMap(cfg)
    tab = cpu.odds_table()  # [21][nRho], row 10 = the centre kind
    assert tab[10, 1] >= 0.5 and tab[10, cfg.am_n_Rho - 2] < 0.5  # (a saturating chain and one that never leaves early)
    for k, n in enumerate(counts):
        xyz = _frame(cfg, n, k)
        gpu.update_map_points(xyz, *IDENT)
        cpu.update_points(xyz, *IDENT)
        what = f"hit_tab_n {tab_n}, {n} copies"
        if record:
            _check_hits(gpu, cpu, what)
            cells, odds = cpu.hit_cells_sorted()
            assert len(cells) > 3  # (the far point spreads: neighbour kinds are covered)
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), what)
    assert gpu.frame_stats()["n_sector_fallbacks"] == 0
    gpu.close()


@pytest.mark.parametrize("tab_n", [None, 0], ids=["default", "tab0"])
def test_cell_with_enough_strong_contributions_takes_the_constant(knobs, tab_n):
    """64 points, 32 each in two neighbouring range steps where the spread reaches one step and the centre odd is >= 0.75: both centre
    cells collect two kinds and 32 strong contributions (strength sum 64 >= MLM_SEC_STRONG_ENOUGH) — 1.0f in any order, the increment
    is mlm_logit(1.0f), from the table's kernel or evaluated in place"""
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    cfg = S1
    if tab_n is not None:
        knobs.set("hit_tab_n", tab_n)
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_points=4096, record_awareness=True, max_batch=2), OracleMap(cfg)
    tab = cpu.odds_table()
    r0 = next(r for r in range(2, cfg.am_n_Rho - 3) if tab[10, r] < 0.86)  # (3 sigma beyond one range step: less than 1.5 sigma inside the cell)
    assert tab[10, r0] >= 0.75 and tab[10, r0 + 1] >= 0.75, (r0, tab[10, r0], tab[10, r0 + 1])
    theta = math.radians(33.4)
    xyz = np.repeat(np.array([_point(cfg, r0, theta), _point(cfg, r0 + 1, theta)]), 32, axis=0)
    gpu.update_map_points(xyz, *IDENT)
    cpu.update_points(xyz, *IDENT)
    _check_hits(gpu, cpu, "saturated cells")
    cells, odds = cpu.hit_cells_sorted()
    assert len(cells) >= 4 and int((odds == np.float32(1.0)).sum()) >= 2  # (both points spread; both centre cells saturate)
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "saturated cells")
    gpu.close()


def test_frontier_mode_handle(knobs):
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    cfg = S1.with_(use_exploration_frontiers=True)
    knobs.set("hit_tab_n", 4)
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_points=4096, max_batch=2), OracleMap(cfg)
    for k, n in enumerate((3, 4, 5, 40)):
        xyz = _frame(cfg, n, k)
        gpu.update_map_points(xyz, *IDENT)
        cpu.update_points(xyz, *IDENT)
        _check_hits(gpu, cpu, f"frontier mode, {n} copies")
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"frontier mode, {n} copies")
        assert np.array_equal(gpu.export_frontier(), cpu.export_frontier())
    gpu.close()
