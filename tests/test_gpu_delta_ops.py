"""mlm_delta_blocks in random operation sequences (in the manner of tests/test_gpu_age_ops.py): integrate / set-free / inflate / crop /
fuse a third handle's dump / age / warp-replace with random arguments on handle A; after every step a delta against the table of the
step before — with a random key box and MLM_DELTA_NO_INFL now and then, held to the contract in numpy (tests/delta_ref.py) on A's raw
export — and the full delta applied to a replica B, whose sorted export then equals A's byte for byte in all three planes."""
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from tests import delta_ref as ref
from tests import warp_ref
from tests.test_gpu_delta import PLANES, check_delta
from tests.test_gpu_warp import small_cfg

pytestmark = pytest.mark.gpu
EXTRA = [int(x) for x in os.environ.get("MLM_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak
SEEDS = [3, 8, 13, 18]
SEQ_N = {3: 3, 8: 8, 13: 3, 18: 8}
FUSE_MODES = ("add", "max", "take", "fill")


@pytest.mark.parametrize("seed", SEEDS + EXTRA)
def test_random_sequences(seed):
    from mlmapping_amd.mlmap import MLMap

    n = SEQ_N.get(seed, (8, 3)[seed % 2])
    cfg = small_cfg(n)
    rng = np.random.default_rng(1000 * seed + 29)
    a, b, c = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    base, traj, traj_c = syn.room_depth(cfg), syn.smooth_trajectory(32, seed), syn.smooth_trajectory(32, seed + 100)
    for j in range(2):
        c.update_map(syn.jitter_depth(base, j, seed=seed + 100), *traj_c[j])
    rows = c.export_blocks()
    d_glb, k, log, prev = n * cfg.subbox_d_xyz, 0, [], None
    seen = {"changed": 0, "new": 0, "gone": 0, "unchanged": 0, "partial": 0}
    ops = ["integrate", "set_free", "integrate", "inflate", "age", "fuse", "crop", "warp", "integrate"] + list(rng.choice(
        ["integrate", "set_free", "crop", "fuse", "age", "warp"], size=5, p=[0.25, 0.2, 0.15, 0.15, 0.15, 0.1]))
    for step, op in enumerate(ops):
        log.append(op)
        what = f"seed {seed}, n {n}, step {step}: {log}"
        q, t = traj[k]
        if op == "integrate":
            a.update_map(syn.jitter_depth(base, k, seed=seed), q, t)
            k += 1
        elif op == "inflate":
            a.inflate_map(t)
        elif op == "set_free":
            held = a.export_blocks()["keys"]
            if len(held):
                lo = held[rng.integers(0, len(held))].astype(np.float64) * d_glb + rng.uniform(0.1, 0.4, 3) * d_glb
                a.setFree_map_in_bound(lo, lo + rng.uniform(0.1, 0.5, 3) * d_glb)
        elif op == "crop":
            ctr = np.floor(t / d_glb).astype(np.int64) + rng.integers(-2, 3, 3)
            w = rng.integers(2, 6, 3)
            a.crop_blocks(ctr - w, 2 * w + 1)
        elif op == "fuse":
            a.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=FUSE_MODES[rng.integers(0, 4)])
        elif op == "age":
            a.age_blocks(mode="step", amount=float(np.float32(rng.uniform(0.05, 1.2))), forget=float(np.float32(rng.uniform(0.0, 1.0))), drop=True,
                         clear_infl=bool(rng.random() < 0.3))
        else:
            a.warp_blocks(warp_ref.make_T(warp_ref.rot(float(rng.uniform(-20, 20))), tuple(rng.uniform(-0.3, 0.3, 3))), replace=True)
        now = a.export_blocks(raw=True)
        table = None if prev is None else prev.table
        if rng.random() < 0.5:  # a partial look: a key box, infl ignored now and then (its previous table is computed by the contract)
            ctr = np.floor(t / d_glb).astype(np.int64) + rng.integers(-1, 2, 3)
            w = rng.integers(0, 3, 3)
            no_infl = bool(rng.random() < 0.5)
            box = (ctr - w, 2 * w + 1)
            p = table if not no_infl or table is None else (table[0], before_no_infl)
            check_delta(a.delta(prev=p, box=box, no_infl=no_infl), ref.delta(now, p, box[0], box[1], no_infl), what + " partial")
            seen["partial"] += 1
        want = ref.delta(now, table)
        d = a.delta(prev=prev, device=bool(step % 2))
        check_delta(d, want, what)
        b.apply_delta(d)
        if step % 2:  # (the contract in numpy reads the table too: the next step hands it back from host memory)
            d.table = tuple(x.cpu().numpy() for x in d.table)
            d.table = (d.table[0], d.table[1].view(np.uint64))
        prev = d
        before_no_infl = ref.delta(now, no_infl=True)["table"][1]
        ea, eb = a.export_blocks(), b.export_blocks()
        for p in PLANES:
            assert ea[p].tobytes() == eb[p].tobytes(), f"{what}: replica {p}"
        sm = want["summary"]
        seen["changed"] += int(sm[5]); seen["new"] += int(sm[6]); seen["gone"] += int(sm[7]); seen["unchanged"] += int(sm[4])
    assert all(v > 0 for v in seen.values()), (seen, log)
    a.close(), b.close(), c.close()
