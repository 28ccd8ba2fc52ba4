"""Rate of mlm_fuse_blocks beside the two ways to fuse a block dump into a live map without it:
  (a) host:   export_blocks of the whole map to the host, the numpy rule of tests/fuse_ref.py, a crop of everything, import_blocks;
  (b) detour: the device path built from calls that existed before — export_block_keys_dev, the key union in torch, merge_pack, a torch
              add of the incoming rows, merge_finish, import_blocks (log-odds and classes only: the merge calls carry no infl).

The maps: 64 frames of the S1 corridor stream, and the crafted map of 16 384 blocks tools/crop_rate.py and tools/warp_rate.py use; both
made consistent first (seen voxels inside the clamp range with occ == 'o' iff L > occupied_sh, unseen ones +0.0f), since only there
does (b) compute what MLM_FUSE_ADD computes.  The dumps: consistent rows over 10 % and over 100 % of the map's blocks, and as many rows
as the 10 % dump with keys the map does not hold.  Device in.  Per map and dump, in ONE loop that alternates the calls, each timed with
the host clock around call + synchronise:
  - fuse_add_ms:      MLM_FUSE_ADD (before every timed call the handle is put back, not timed: everything dropped, the snapshot imported);
  - fuse_dry_ms:      MLM_FUSE_DRY, the diff;
  - fuse_add_rows_ms: MLM_FUSE_ADD with per_row (into host memory, staged);
  - host_ms, detour_ms: the comparators (the handle is put back afterwards).
Before anything is timed both comparators must leave the map the call leaves (sorted exports; (b) without infl).  Every fuse row reports
the bytes the rule must move — per voxel of a touching row 2 read by the probe, then 12 read and at most 6 written by the apply (no
stores for the diff) — and the bytes/s that makes of the median, beside the HBM peak.
Writes one JSON document.  Usage: python tools/fuse_rate.py [--reps 30] [--warmup 2] [--cmp-reps 2] [--out profiles/fuse_rate.json]"""
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
from tests import fuse_ref as ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
WHOLE = ([ref.KEY_MIN] * 3, [1 << 21] * 3)
MAX_BLOCKS = 16384
PLANES = ("keys", "log_odds", "occ", "infl")


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


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cmp-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_rate.json"))
    a = ap.parse_args()
    cfg = S1
    C = cfg.cells_per_block
    lim = (cfg.lm_log_odds_min, cfg.lm_log_odds_max, cfg.lm_occupied_sh)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    out = {"hbm_peak_GBs": HBM_PEAK_GBS, "reps": a.reps, "warmup": a.warmup, "maps": {}, "cases": {},
           "not_measured": ["frontier-mode handles (only the diff runs there)", "subbox_n other than 10", "host sources (staged whole)",
                            "MLM_FUSE_MAX / TAKE / FILL (the same reads, fewer stores)", "per_row in device memory", "unaligned sources (the narrow lane path)",
                            "a fuse that has to grow the pool", "maps that are not consistent (the detour computes something else there)"]}

    def dev(b):
        return {k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in PLANES}

    def pack(k):
        k = k.long() + (1 << 20)
        return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]

    def run_map(tag, m, reps, cmp_reps):
        whole = m.export_blocks()
        nb = len(whole["keys"])
        out["maps"][tag].update(blocks=nb, cells=C, map_bytes=nb * (12 + 6 * C))
        snap = dev(whole)
        sync()

        def restore():
            m.crop_blocks(*WHOLE, inside=True)
            m.import_blocks((snap["keys"].data_ptr(), nb), snap["log_odds"].data_ptr(), snap["occ"].data_ptr(), snap["infl"].data_ptr())

        def host_way(rows):
            t0 = time.perf_counter()
            w, _, _ = ref.fuse(m.export_blocks(raw=True), rows, ref.ADD, lim=lim)
            m.crop_blocks(*WHOLE, inside=True)
            m.import_blocks(w["keys"], w["log_odds"], w["occ"], w["infl"])
            sync()
            return (time.perf_counter() - t0) * 1e3

        def detour(d, nr):
            t0 = time.perf_counter()
            held = m.block_count()
            km = torch.empty((held, 3), dtype=torch.int32, device="cuda")
            sync()
            m.export_block_keys_dev(km.data_ptr(), held)
            u, inv = torch.unique(pack(torch.cat([km, d["keys"]])), return_inverse=True)
            uk = torch.stack([(u >> 42) - (1 << 20), ((u >> 21) & 0x1FFFFF) - (1 << 20), (u & 0x1FFFFF) - (1 << 20)], dim=1).to(torch.int32).contiguous()
            U = uk.shape[0]
            lo = torch.empty((U, C), dtype=torch.float32, device="cuda")
            seen = torch.empty((U, C), dtype=torch.uint8, device="cuda")
            occ = torch.empty((U, C), dtype=torch.uint8, device="cuda")
            sync()
            m.merge_pack(uk.data_ptr(), U, lo.data_ptr(), seen.data_ptr())
            idx = inv[held:]
            lo[idx] += d["log_odds"]
            seen[idx] |= (d["occ"] != ref.U).to(torch.uint8)
            sync()
            m.merge_finish(lo.data_ptr(), seen.data_ptr(), U * C, occ.data_ptr())
            m.import_blocks((uk.data_ptr(), U), lo.data_ptr(), occ.data_ptr())
            sync()
            return (time.perf_counter() - t0) * 1e3

        tenth = max(1, nb // 10)
        fresh = whole["keys"][rng.permutation(nb)[:tenth]] + np.array([0, 0, 4096], dtype=np.int32)  # (keys far above every block of the map)
        dumps = {"tenth": whole["keys"][rng.permutation(nb)[:tenth]], "all": whole["keys"][rng.permutation(nb)], "new": fresh}
        for name, keys in dumps.items():
            rows = consistent(rng, keys, C, lim)
            nr = len(keys)
            d = dev(rows)
            sync()
            src = ((d["keys"].data_ptr(), nr), d["log_odds"].data_ptr(), d["occ"].data_ptr(), d["infl"].data_ptr())
            # the same map on all three sides before anything is timed
            res = m.fuse_blocks(*src)
            got = m.export_blocks()
            restore()
            host_way(rows)
            via_host = m.export_blocks()
            restore()
            detour(d, nr)
            via_detour = m.export_blocks()
            restore()
            assert all(got[k].tobytes() == via_host[k].tobytes() for k in PLANES), "the host comparator computes another map"
            assert all(got[k].tobytes() == via_detour[k].tobytes() for k in ("keys", "log_odds", "occ")), "the device detour computes another map"
            ts = {"fuse_add_ms": [], "fuse_dry_ms": [], "fuse_add_rows_ms": [], "host_ms": [], "detour_ms": []}
            summary = [int(v) for v in res["summary"]]
            for r in range(a.warmup + reps):
                for k, kw in (("fuse_add_ms", {}), ("fuse_dry_ms", dict(dry=True)), ("fuse_add_rows_ms", dict(per_row=True))):
                    sync()
                    t0 = time.perf_counter()
                    m.fuse_blocks(*src, **kw)
                    sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    if k != "fuse_dry_ms":
                        restore()
                    if r >= a.warmup:
                        ts[k].append(dt)
                sync()
                dt = detour(d, nr)
                restore()
                if r >= a.warmup:
                    ts["detour_ms"].append(dt)
                if len(ts["host_ms"]) < cmp_reps:  # (in the same loop; up to seconds per call, so fewer of them and no warm-up)
                    ts["host_ms"].append(host_way(rows))
                    restore()
            row = {k: stats(v) for k, v in ts.items() if v}
            touching = nr - summary[3]
            for k in ("fuse_add_ms", "fuse_dry_ms", "fuse_add_rows_ms"):
                med = row[k]["median"]
                b = touching * C * (14 if k == "fuse_dry_ms" else 20)
                row[k].update(rule_bytes=b, achieved_GBs=b / (med * 1e-3) / 1e9, fraction_of_hbm_peak=b / (med * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              host_over_call=row["host_ms"]["median"] / med, detour_over_call=row["detour_ms"]["median"] / med)
            row.update(rows=nr, summary=summary)
            out["cases"][f"{tag}_{name}"] = row
            print(tag, name, json.dumps({k: v["median"] for k, v in row.items() if isinstance(v, dict)}), flush=True)

    def make_consistent(m):
        b = m.export_blocks()
        seen = b["occ"] != ref.U
        lo = np.where(seen, ref.clamp(b["log_odds"], lim), np.float32(0.0)).astype(np.float32)
        occ = np.where(seen, np.where(lo > np.float32(lim[2]), ref.O, ref.F), ref.U).astype(np.uint8)
        m.crop_blocks(*WHOLE, inside=True)
        m.import_blocks(b["keys"], lo, occ, b["infl"])

    out["maps"]["corridor"] = {"config": "S1", "scene": "corridor", "frames": 64}
    m = MLMap(cfg, max_blocks=MAX_BLOCKS, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    make_consistent(m)
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
