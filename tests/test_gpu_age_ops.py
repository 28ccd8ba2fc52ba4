"""mlm_age_blocks in random operation sequences (in the manner of tests/test_gpu_fuse_ops.py): integrate / set-free / crop / fuse a third
handle's dump / age with random arguments on handle A, mirrored on a twin handle B for which every aging and every fuse is done by the
definition — B's raw export through the contract in numpy (tests/age_ref.py, tests/fuse_ref.py), a crop of everything, import_blocks of
the result.  After every aging, crop and fuse A's raw export equals the numpy reference of its raw export before; after every step both
sorted exports are identical, float bits included.  At the end two read-outs of the aged map, export_window and export_esdf, against
their references."""
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from tests import age_ref as ref
from tests import crop_ref, esdf_ref, fuse_ref
from tests.test_gpu_esdf import check as check_esdf
from tests.test_gpu_fuse import fuse_by_definition, same
from tests.test_gpu_warp import empty, small_cfg

pytestmark = pytest.mark.gpu
EXTRA = [int(x) for x in os.environ.get("MLM_AGE_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak
AGE_SEEDS = [3, 4, 7, 10]
AGE_SEQ_N = {3: 3, 4: 4, 7: 7, 10: 8}
FUSE_MODES = ("add", "max", "take", "fill")


def age_by_definition(b, kw):
    want, sm, _ = ref.age(b.export_blocks(raw=True), **kw)
    empty(b)
    if len(want["keys"]):
        b.import_blocks(want["keys"], want["log_odds"], want["occ"], want["infl"])
    return sm


def dense(b, lo, dims, n):
    """the occ / infl classes of a voxel box as export_window reports them (0 OCCUPIED, 1 FREE, -1 UNKNOWN; infl 0 or -1), from an export"""
    iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
    v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
    g = np.floor_divide(v, n)
    c = v - g * n
    cid = c[:, 2] * n * n + c[:, 1] * n + c[:, 0]
    at = {tuple(k): i for i, k in enumerate(b["keys"].tolist())}
    row = np.array([at.get(tuple(k), -1) for k in g.tolist()], dtype=np.int64)
    have = row >= 0
    occ_b = np.where(have, b["occ"][np.maximum(row, 0), cid], ref.U)
    infl_b = np.where(have, b["infl"][np.maximum(row, 0), cid], ref.U)
    shape = (dims[2], dims[1], dims[0])
    return (np.where(occ_b == ref.O, 0, np.where(occ_b == ref.F, 1, -1)).reshape(shape), np.where(infl_b == ref.O, 0, -1).reshape(shape))


@pytest.mark.parametrize("seed", AGE_SEEDS + EXTRA)
def test_random_sequences(seed):
    from mlmapping_amd.mlmap import MLMap

    n = AGE_SEQ_N.get(seed, (4, 3)[seed % 2])
    cfg = small_cfg(n)
    rng = np.random.default_rng(1000 * seed + 17)
    a, b, c = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    base, traj, traj_c = syn.room_depth(cfg), syn.smooth_trajectory(32, seed), syn.smooth_trajectory(32, seed + 100)
    for j in range(2):
        c.update_map(syn.jitter_depth(base, j, seed=seed + 100), *traj_c[j])
    rows = c.export_blocks()
    d_glb, k, log, aged, dropped = n * cfg.subbox_d_xyz, 0, [], 0, 0
    ops = ["integrate", "age", "integrate", "inflate", "age", "fuse", "age", "set_free", "crop", "age", "integrate", "age"] + list(rng.choice(
        ["integrate", "set_free", "crop", "fuse", "age"], size=8, p=[0.2, 0.1, 0.1, 0.15, 0.45])) + ["age"]
    for step, op in enumerate(ops):
        log.append(op)
        what = f"seed {seed}, n {n}, step {step}: {log}"
        q, t = traj[k]
        if op == "integrate":
            img = syn.jitter_depth(base, k, seed=seed)
            a.update_map(img, q, t), b.update_map(img, q, t)
            k += 1
        elif op == "inflate":
            a.inflate_map(t), b.inflate_map(t)
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
            before = a.export_blocks(raw=True)
            a.crop_blocks(ctr - w, 2 * w + 1), b.crop_blocks(ctr - w, 2 * w + 1)
            kept, _, _ = crop_ref.crop({p: before[p] for p in ("keys", "log_odds", "occ", "infl")}, ctr - w, 2 * w + 1, inside=False)
            same(a.export_blocks(raw=True), kept, what)
        elif op == "fuse":
            mode = FUSE_MODES[rng.integers(0, 4)]
            before = a.export_blocks(raw=True)
            want, sm, _ = fuse_ref.fuse(before, rows, mode)
            res = a.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=mode)
            assert res["summary"].tolist() == sm.tolist(), what
            same(a.export_blocks(raw=True), want, what)
            fuse_by_definition(b, rows, mode)
        else:
            kw = dict(mode=("scale", "step")[rng.integers(0, 2)], drop=bool(rng.random() < 0.7), clear_infl=bool(rng.random() < 0.3), outside=bool(rng.random() < 0.5))
            kw["amount"] = float(np.float32(rng.uniform(0.3, 0.95) if kw["mode"] == "scale" else rng.uniform(0.05, 1.2)))
            kw["forget"] = float(np.float32(rng.uniform(0.0, 1.0))) if rng.random() < 0.7 else None
            if rng.random() < 0.6:
                ctr = np.floor(t / d_glb).astype(np.int64) + rng.integers(-1, 2, 3)
                w = rng.integers(0, 3, 3)
                kw.update(key_lo=ctr - w, key_dims=2 * w + 1)
            before = a.export_blocks(raw=True)
            want, sm, pr = ref.age(before, **kw)
            if rng.random() < 0.3:
                res = a.age_blocks(dry=True, per_block=True, **kw)
                assert res["summary"].tolist() == sm.tolist() and res["per_block"].tolist() == pr.tolist(), what
                same(a.export_blocks(raw=True), before, what)
            res = a.age_blocks(per_block=True, **kw)
            assert res["summary"].tolist() == sm.tolist() and res["per_block"].tolist() == pr.tolist(), (what, kw, res["summary"].tolist(), sm.tolist())
            same(a.export_blocks(raw=True), want, what)
            assert age_by_definition(b, kw).tolist() == sm.tolist(), what
            aged += sm[4] > 0
            dropped += int(sm[2])
        ea, eb = a.export_blocks(), b.export_blocks()
        same(ea, eb, what)
        assert a.block_count() == len(ea["keys"]), what
        if op in ("integrate", "age", "crop", "fuse"):  # (mlm_frame_stats follows the frames and the block calls; inflate_map may create blocks)
            assert a.frame_stats()["n_blocks"] == len(ea["keys"]), what
    assert aged >= 4 and k >= 3, (aged, dropped, log)
    # two read-outs of the aged map: the window's classes from the export in numpy and its odds from the twin; the distance field from
    # the classes of the box grown by C (tests/esdf_ref.py)
    e = a.export_blocks()
    if len(e["keys"]):
        lo = [int(v) for v in e["keys"].min(0) * n - 3]
        dims = [int(v) for v in np.minimum((e["keys"].max(0) + 1) * n + 2 - np.array(lo), 40)]
        w, wb = a.export_window(lo, dims, odds=True, occ=True, infl=True), b.export_window(lo, dims, odds=True, occ=True, infl=True)
        occ, infl = dense(e, lo, dims, n)
        assert np.array_equal(w["occ"].astype(np.int64), occ) and np.array_equal(w["infl"].astype(np.int64), infl)
        assert np.array_equal(w["odds"].view(np.uint32), wb["odds"].view(np.uint32))
        C = 4
        glo, gdims = esdf_ref.grown(lo, dims, C)
        gocc, ginfl = dense(e, glo, gdims, n)
        flags = esdf_ref.OCC | esdf_ref.INFL
        exp = esdf_ref.expected(esdf_ref.classes_mask(gocc, ginfl, flags), C, False, cfg.subbox_d_xyz)
        got = a.export_esdf(lo, dims, C, occ=True, infl=True, sqdist=True, dist=True, grad=True)
        check_esdf(got, exp, f"seed {seed}")
    a.close(), b.close(), c.close()
