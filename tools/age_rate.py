"""Rate of mlm_age_blocks beside the two ways to age a map without it:
  (a) host:   export_blocks of the whole map to the host, the numpy rule of tests/age_ref.py, a crop of everything, import_blocks;
  (b) detour: the device path built from calls that existed before — export_block_keys_dev, merge_pack, a torch multiply of the rows,
              merge_finish, import_blocks.  Log-odds and classes only: it forgets nothing, drops nothing and never touches infl, so it
              stands beside MLM_AGE_SCALE without flags alone.

The maps: 64 frames of the S1 corridor stream, and the crafted map of 16 384 blocks tools/crop_rate.py, warp_rate.py and fuse_rate.py use;
both made consistent first (seen voxels inside the clamp range with occ == 'o' iff L > occupied_sh, unseen ones +0.0f), since only
there does (b) compute what MLM_AGE_SCALE computes.  Per map two variants: about 10 % and about 50 % of the blocks, chosen at random,
rewritten as faint blocks (|log-odds| <= 0.2, no infl) that SCALE by 0.9 with FORGET 0.25 empties.  Device in place.  Per map and
variant, in ONE loop that alternates the calls, each timed with the host clock around call + synchronise:
  - age_scale_ms:       MLM_AGE_SCALE by 0.9 over every block (before every timed mutating call the handle is put back, not timed:
                        everything dropped, the snapshot imported);
  - age_forget_drop_ms: the same with MLM_AGE_FORGET 0.25 and MLM_AGE_DROP;
  - age_dry_ms:         that call with MLM_AGE_DRY;
  - age_rows_ms:        MLM_AGE_SCALE with per_block into host memory (staged);
  - host_ms (against the FORGET + DROP call), detour_ms (against the SCALE call): the comparators, the handle put back afterwards.
Before anything is timed each comparator must leave the map its call leaves (sorted exports; (b): keys, log-odds and classes).  Every
age row reports the bytes by the rule's own count — 6 read and at most 6 written per voxel of a selected block (no stores for the dry
call), plus 2 (12 + 6 cells) per block the drop can move at most — and the bytes/s that makes of the median, beside the HBM peak.
Writes one JSON document.  Usage: python tools/age_rate.py [--reps 30] [--warmup 2] [--cmp-reps 2] [--out profiles/age_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd import synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402
from tests import age_ref as ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
KEY_MIN = -(1 << 20)
WHOLE = ([KEY_MIN] * 3, [1 << 21] * 3)
MAX_BLOCKS = 16384
PLANES = ("keys", "log_odds", "occ", "infl")
AMOUNT, FORGET = 0.9, 0.25


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


def consistent(rng, keys, C, lim):
    nb = len(keys)
    lo = ref.clamp(rng.uniform(-3.0, 5.0, size=(nb, C)).astype(np.float32), lim)
    seen = rng.random((nb, C)) < 0.6
    lo[~seen] = np.float32(0.0)
    occ = np.where(seen, np.where(lo > np.float32(lim[2]), ref.O, ref.F), ref.U).astype(np.uint8)
    return {"keys": np.ascontiguousarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": lo, "occ": occ,
            "infl": rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(nb, C))}


def with_faint(rng, whole, frac):
    """the map with a random `frac` of its blocks rewritten as faint ones: free voxels of |log-odds| <= 0.2, no infl"""
    b = {k: np.array(whole[k], copy=True) for k in PLANES}
    nb, C = b["log_odds"].shape
    pick = rng.permutation(nb)[:max(1, int(round(frac * nb)))]
    lo = rng.uniform(-0.2, 0.2, size=(len(pick), C)).astype(np.float32)
    seen = rng.random((len(pick), C)) < 0.6
    lo[~seen] = np.float32(0.0)
    b["log_odds"][pick], b["occ"][pick], b["infl"][pick] = lo, np.where(seen, ref.F, ref.U).astype(np.uint8), ref.U
    return b


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cmp-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "age_rate.json"))
    a = ap.parse_args()
    cfg = S1
    C = cfg.cells_per_block
    lim = (cfg.lm_log_odds_min, cfg.lm_log_odds_max, cfg.lm_occupied_sh)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    out = {"hbm_peak_GBs": HBM_PEAK_GBS, "reps": a.reps, "warmup": a.warmup, "amount": AMOUNT, "forget": FORGET, "maps": {}, "cases": {},
           "not_measured": ["MLM_AGE_STEP (the same reads and stores)", "a key box or MLM_AGE_OUTSIDE (an unselected block costs one key read)",
                            "MLM_AGE_CLEAR_INFL (one more dword store per four voxels)", "subbox_n other than 10 (the one-voxel lane path of subbox_n 2, 3, 5, 7, 9)",
                            "per_block in device memory", "maps that are not consistent (the detour computes something else there)",
                            "calls while frames are in flight (the call drains them first)", "the kernels on their own (host clock around the whole call only)"]}

    def dev(b):
        return {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in PLANES}

    def run_variant(tag, m, variant, reps, cmp_reps):
        nb = len(variant["keys"])
        snap = dev(variant)
        sync()

        def restore():
            m.crop_blocks(*WHOLE, inside=True)
            m.import_blocks((snap["keys"].data_ptr(), nb), snap["log_odds"].data_ptr(), snap["occ"].data_ptr(), snap["infl"].data_ptr())

        def host_way():
            t0 = time.perf_counter()
            w, _, _ = ref.age(m.export_blocks(raw=True), mode=ref.SCALE, amount=AMOUNT, forget=FORGET, drop=True, lim=lim)
            m.crop_blocks(*WHOLE, inside=True)
            if len(w["keys"]):
                m.import_blocks(w["keys"], w["log_odds"], w["occ"], w["infl"])
            sync()
            return (time.perf_counter() - t0) * 1e3

        def detour():
            t0 = time.perf_counter()
            held = m.block_count()
            km = torch.empty((held, 3), dtype=torch.int32, device="cuda")
            lo = torch.empty((held, C), dtype=torch.float32, device="cuda")
            seen = torch.empty((held, C), dtype=torch.uint8, device="cuda")
            occ = torch.empty((held, C), dtype=torch.uint8, device="cuda")
            sync()
            m.export_block_keys_dev(km.data_ptr(), held)
            m.merge_pack(km.data_ptr(), held, lo.data_ptr(), seen.data_ptr())
            lo *= AMOUNT
            sync()
            m.merge_finish(lo.data_ptr(), seen.data_ptr(), held * C, occ.data_ptr())
            m.import_blocks((km.data_ptr(), held), lo.data_ptr(), occ.data_ptr())
            sync()
            return (time.perf_counter() - t0) * 1e3

        calls = {"age_scale_ms": dict(), "age_forget_drop_ms": dict(forget=FORGET, drop=True), "age_dry_ms": dict(forget=FORGET, drop=True, dry=True),
                 "age_rows_ms": dict(per_block=True)}
        # the same map on every side before anything is timed
        restore()
        summaries = {}
        for k in ("age_scale_ms", "age_forget_drop_ms"):
            summaries[k] = [int(v) for v in m.age_blocks(mode="scale", amount=AMOUNT, **calls[k])["summary"]]
            got = m.export_blocks()
            restore()
            if k == "age_scale_ms":
                detour()
                via = m.export_blocks()
                assert all(got[p].tobytes() == via[p].tobytes() for p in ("keys", "log_odds", "occ")), "the device detour computes another map"
            else:
                host_way()
                via = m.export_blocks()
                assert all(got[p].tobytes() == via[p].tobytes() for p in PLANES), "the host comparator computes another map"
            restore()
        ts = {k: [] for k in list(calls) + ["host_ms", "detour_ms"]}
        for r in range(a.warmup + reps):
            for k, kw in calls.items():
                sync()
                t0 = time.perf_counter()
                m.age_blocks(mode="scale", amount=AMOUNT, **kw)
                sync()
                dt = (time.perf_counter() - t0) * 1e3
                if k != "age_dry_ms":
                    restore()
                if r >= a.warmup:
                    ts[k].append(dt)
            sync()
            dt = detour()
            restore()
            if r >= a.warmup:
                ts["detour_ms"].append(dt)
            if len(ts["host_ms"]) < cmp_reps:  # (in the same loop; up to seconds per call, so fewer of them and no warm-up)
                ts["host_ms"].append(host_way())
                restore()
        row = {k: stats(v) for k, v in ts.items() if v}
        D = summaries["age_forget_drop_ms"][2]
        for k in calls:
            med = row[k]["median"]
            b = nb * C * (6 if k == "age_dry_ms" else 12) + (2 * min(D, nb - D) * (12 + 6 * C) if k == "age_forget_drop_ms" else 0)
            cmp_key = "detour_ms" if k in ("age_scale_ms", "age_rows_ms") else "host_ms"
            row[k].update(rule_bytes=b, achieved_GBs=b / (med * 1e-3) / 1e9, fraction_of_hbm_peak=b / (med * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          comparator=cmp_key, comparator_over_call=row[cmp_key]["median"] / med)
        row.update(blocks=nb, emptied_blocks=D, summary_scale=summaries["age_scale_ms"], summary_forget_drop=summaries["age_forget_drop_ms"])
        out["cases"][tag] = row
        print(tag, json.dumps({k: v["median"] for k, v in row.items() if isinstance(v, dict)}), flush=True)

    def run_map(tag, m, reps, cmp_reps):
        b = m.export_blocks()
        seen = b["occ"] != ref.U
        lo = np.where(seen, ref.clamp(b["log_odds"], lim), np.float32(0.0)).astype(np.float32)
        occ = np.where(seen, np.where(lo > np.float32(lim[2]), ref.O, ref.F), ref.U).astype(np.uint8)
        whole = {"keys": b["keys"], "log_odds": lo, "occ": occ, "infl": b["infl"]}
        nb = len(whole["keys"])
        out["maps"][tag].update(blocks=nb, cells=C, map_bytes=nb * (12 + 6 * C))
        for name, frac in (("p10", 0.1), ("p50", 0.5)):
            run_variant(f"{tag}_{name}", m, with_faint(rng, whole, frac), reps, cmp_reps)

    out["maps"]["corridor"] = {"config": "S1", "scene": "corridor", "frames": 64}
    m = MLMap(cfg, max_blocks=MAX_BLOCKS, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    run_map("corridor", m, a.reps, min(a.reps, 5 * a.cmp_reps))
    m.close()
    out["maps"]["crafted"] = {"config": "S1", "scene": "32 x 32 x 16 block keys, consistent random planes"}
    big = MLMap(cfg, max_blocks=4 * MAX_BLOCKS, max_batch=8)
    kx, ky, kz = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing="ij")
    keys = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.int32)[rng.permutation(MAX_BLOCKS)]
    c = consistent(rng, keys, C, lim)
    big.import_blocks(c["keys"], c["log_odds"], c["occ"], c["infl"])
    run_map("crafted", big, max(3, a.reps // 3), a.cmp_reps)
    big.close()
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
