"""mlm_warp_blocks in random operation sequences (in the manner of tests/test_gpu_query_ops.py): integrate / set-free / crop /
warp-and-compare / reanchor on handle A, mirrored on a twin handle B for which every reanchor is done by the definition — B's export
through the contract in numpy (tests/warp_ref.py), a crop of everything, import_blocks of the result.  After every step both sorted
exports are identical, float bits included, and a warp of A into host arrays equals the numpy rule over A's export."""
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from tests import warp_ref as ref
from tests.test_gpu_warp import empty, same, same_counts, small_cfg

pytestmark = pytest.mark.gpu
EXTRA = [int(x) for x in os.environ.get("MLM_WARP_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak
WARP_SEEDS = [4, 9]
WARP_SEQ_N = {4: 4, 9: 9}


def random_T(rng, whole):
    """a correction as a matcher finds it — a degree or two, a few voxels — or a whole-voxel shift"""
    if whole:
        return ref.make_T(None, rng.integers(-6, 7, 3).astype(np.float64) * 0.1)
    yaw, pitch, roll = rng.uniform(-3, 3), rng.uniform(-1, 1), rng.uniform(-1, 1)
    return ref.make_T(ref.rot(yaw, pitch, roll), rng.uniform(-0.35, 0.35, 3))


@pytest.mark.parametrize("seed", WARP_SEEDS + EXTRA)
def test_random_sequences(seed):
    from mlmapping_amd.mlmap import MLMap, invert_T

    n = WARP_SEQ_N.get(seed, (4, 9)[seed % 2])
    cfg = small_cfg(n)
    rng = np.random.default_rng(1000 * seed + 7)
    a, b = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    base, traj = syn.room_depth(cfg), syn.smooth_trajectory(32, seed)
    d_glb, k, log, warps, anchors = n * cfg.subbox_d_xyz, 0, [], 0, 0
    ops = ["integrate", "integrate", "warp", "reanchor", "integrate", "set_free", "crop", "warp", "reanchor", "integrate"] + list(rng.choice(
        ["integrate", "set_free", "crop", "warp", "reanchor"], size=6, p=[0.3, 0.15, 0.15, 0.2, 0.2]))
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
            c = np.floor(t / d_glb).astype(np.int64) + rng.integers(-2, 3, 3)
            w = rng.integers(2, 6, 3)
            a.crop_blocks(c - w, 2 * w + 1), b.crop_blocks(c - w, 2 * w + 1)
        elif op == "warp":
            T = random_T(rng, bool(rng.random() < 0.3))
            seen = bool(rng.random() < 0.5)
            cur = a.export_blocks()
            want = ref.warp(cur, T, n, cfg.subbox_d_xyz, seen=seen)
            res = a.warp_blocks(T, seen=seen, out=True)
            same(res, want, what)
            same_counts(res["summary"], want["summary"], what)
            warps += len(want["keys"]) > 0
        else:
            T_ds = random_T(rng, bool(rng.random() < 0.3))
            cur = b.export_blocks()
            want = ref.warp(cur, ref.invert(T_ds), n, cfg.subbox_d_xyz)
            assert np.array_equal(invert_T(T_ds), ref.invert(T_ds))
            res = a.reanchor(T_ds)
            same_counts(res["summary"], np.where(np.arange(8) == 3, 0, want["summary"]), what)
            empty(b)
            if len(want["keys"]):
                b.import_blocks(want["keys"], want["log_odds"], want["occ"], want["infl"])
            anchors += len(want["keys"]) > 0
        ea, eb = a.export_blocks(), b.export_blocks()
        same(ea, eb, what)
        assert not ea["collapsed"].any() and a.block_count() == len(ea["keys"]) == a.frame_stats()["n_blocks"], what
    assert warps >= 2 and anchors >= 2 and k >= 4, (warps, anchors, log)
    a.close(), b.close()
