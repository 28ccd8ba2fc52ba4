"""OracleMap.import_blocks (mlo_import_blocks, the counterpart of mlm_import_blocks): a map exported from the oracle and imported
into a fresh one is the same map — the same export, and the same answer bits for every query kind — on S1 and on S1 frontier mode
at n = 5, whose released blocks keep element 0 only (map_local.cpp:221-226).  The crafted maps of tests/test_gpu_query_exact.py
are built this way."""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import assert_same_bits, voxel_centres


@pytest.mark.parametrize("name", ["S1", "S1 frontier n5"])
def test_export_import_roundtrip(name):
    from oracle.binding import OracleMap

    cfg = S1 if name == "S1" else S1.with_(use_exploration_frontiers=True, subbox_n=5)
    src = OracleMap(cfg)
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 5):
        src.update_depth(img, q, t)
    src.inflate_map([0.0, 0.0, 1.5])
    b = src.export_blocks()
    if "frontier" in name:
        assert b["collapsed"].sum() > 20, "the scene should release blocks"
    dst = OracleMap(cfg)
    dst.import_blocks(b["keys"], b["log_odds"], b["occ"], b["infl"], b["collapsed"])
    c = dst.export_blocks()
    for k in ("keys", "collapsed", "occ", "infl"):
        assert np.array_equal(c[k], b[k]), k
    assert np.array_equal(c["log_odds"].view(np.uint32), b["log_odds"].view(np.uint32))
    assert not c["frontier_cnt"].any()  # (frontier sets are not imported)

    rng = np.random.default_rng(7)
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    lo, hi = b["keys"].min(0) * d * n - 1.0, (b["keys"].max(0) + 1) * d * n + 1.0
    edge = rng.uniform(lo, hi, size=(2000, 3))
    edge[:, 0] = np.nextafter(np.round(edge[:, 0] / d) * d, rng.choice([-np.inf, np.inf], 2000))
    pos = np.concatenate([rng.uniform(lo, hi, size=(4000, 3)), voxel_centres(b, cfg, 6000, seed=1), edge])
    assert_same_bits(dst.getOccupancy(pos), src.getOccupancy(pos), "getOccupancy")
    assert_same_bits(dst.getInflateOccupancy(pos), src.getInflateOccupancy(pos), "getInflateOccupancy")
    assert_same_bits(dst.getOdd(pos), src.getOdd(pos), "getOdd")
    for f in (0.05, 0.15, -0.15):
        assert_same_bits(dst.getOccupancy(pos[:3000], inflate=f), src.getOccupancy(pos[:3000], inflate=f), f"getOccupancy({f})")
    for it in (0, 1, 2, 5, 9):
        assert_same_bits(dst.getOddGrad(pos[:4000], it), src.getOddGrad(pos[:4000], it), f"getOddGrad({it})")
    glb = np.concatenate([b["keys"][rng.integers(0, b["keys"].shape[0], 3000)], rng.integers(-60, 60, size=(500, 3)).astype(np.int32)])
    sub = rng.integers(0, cfg.cells_per_block, glb.shape[0]).astype(np.int32)
    assert_same_bits(dst.getOddAt(glb, sub), src.getOddAt(glb, sub), "getOddAt")
