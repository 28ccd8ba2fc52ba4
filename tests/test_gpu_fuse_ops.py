"""mlm_fuse_blocks in random operation sequences (in the manner of tests/test_gpu_warp_ops.py): integrate / set-free / crop / fuse a
third handle's dump in a random mode / fuse_from that handle under a random small transform / a DRY diff on handle A, mirrored on a
twin handle B for which every fuse is done by the definition — B's raw export through the contract in numpy (tests/fuse_ref.py), a crop
of everything, import_blocks of the result.  After every step both sorted exports are identical, float bits included."""
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from tests import fuse_ref as ref
from tests import warp_ref
from tests.test_gpu_fuse import fuse_by_definition, same
from tests.test_gpu_warp import small_cfg
from tests.test_gpu_warp_ops import random_T

pytestmark = pytest.mark.gpu
EXTRA = [int(x) for x in os.environ.get("MLM_FUSE_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak
FUSE_SEEDS = [4, 9]
FUSE_SEQ_N = {4: 4, 9: 9}
MODES = ("add", "max", "take", "fill")


@pytest.mark.parametrize("seed", FUSE_SEEDS + EXTRA)
def test_random_sequences(seed):
    from mlmapping_amd.mlmap import MLMap

    n = FUSE_SEQ_N.get(seed, (4, 9)[seed % 2])
    cfg = small_cfg(n)
    rng = np.random.default_rng(1000 * seed + 11)
    a, b, c = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    base, traj, traj_c = syn.room_depth(cfg), syn.smooth_trajectory(32, seed), syn.smooth_trajectory(32, seed + 100)
    for j in range(3):
        c.update_map(syn.jitter_depth(base, j, seed=seed + 100), *traj_c[j])
    d_glb, k, log, fused, diffs = n * cfg.subbox_d_xyz, 0, [], 0, 0
    ops = ["integrate", "fuse", "integrate", "fuse_from", "diff", "set_free", "crop", "fuse", "integrate", "fuse_from"] + list(rng.choice(
        ["integrate", "set_free", "crop", "fuse", "fuse_from", "diff"], size=6, p=[0.25, 0.1, 0.15, 0.2, 0.2, 0.1]))
    for step, op in enumerate(ops):
        log.append(op)
        what = f"seed {seed}, n {n}, step {step}: {log}"
        q, t = traj[k]
        if op == "integrate":
            img = syn.jitter_depth(base, k, seed=seed)
            a.update_map(img, q, t), b.update_map(img, q, t)
            k += 1
        elif op == "set_free":
            held = a.export_blocks()["keys"]
            if len(held):
                key = held[rng.integers(0, len(held))].astype(np.float64)
                lo = key * d_glb + rng.uniform(0.1, 0.4, 3) * d_glb
                hi = lo + rng.uniform(0.1, 0.5, 3) * d_glb
                a.setFree_map_in_bound(lo, hi), b.setFree_map_in_bound(lo, hi)
        elif op == "crop":
            ctr = np.floor(t / d_glb).astype(np.int64) + rng.integers(-2, 3, 3)
            w = rng.integers(2, 6, 3)
            a.crop_blocks(ctr - w, 2 * w + 1), b.crop_blocks(ctr - w, 2 * w + 1)
        else:
            mode = MODES[rng.integers(0, 4)]
            if op == "fuse_from":
                T = random_T(rng, bool(rng.random() < 0.3))
                rows = warp_ref.warp(c.export_blocks(), T, n, cfg.subbox_d_xyz, seen=True)
            else:
                T, rows = None, c.export_blocks()
            before = a.export_blocks(raw=True)
            want, sm, pr = ref.fuse(before, rows, mode)
            if op == "diff":
                res = a.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=mode, dry=True, per_row=True)
                assert res["per_row"].tolist() == pr.tolist(), what
                same(a.export_blocks(raw=True), before, what)
                diffs += 1
            else:
                res = a.fuse_from(c, T, mode=mode) if op == "fuse_from" else a.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=mode)
                same(a.export_blocks(raw=True), want, what)
                fuse_by_definition(b, rows, mode)
                fused += sm[4] > 0
            assert res["summary"].tolist() == sm.tolist(), what
        ea, eb = a.export_blocks(), b.export_blocks()
        same(ea, eb, what)
        assert a.block_count() == len(ea["keys"]) == a.frame_stats()["n_blocks"], what
    assert fused >= 3 and diffs >= 1 and k >= 3, (fused, diffs, log)
    a.close(), b.close(), c.close()
