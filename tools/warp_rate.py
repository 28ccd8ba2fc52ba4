"""Rate of mlm_warp_blocks beside the only exact way to resample a map without it: export_blocks of the whole map to the host, the
numpy gather of tests/warp_ref.py, import_blocks of the result into the emptied handle.

The maps: 64 frames of the S1 corridor stream, and the crafted map of 16 384 blocks tools/crop_rate.py uses.  The transforms: the
identity, a whole-voxel shift, a yaw of 30 degrees, a general rotation plus translation.  Device in, device out.  Per map and
transform, in ONE loop that alternates the calls, each timed with the host clock around call + synchronise:
  - warp_dev_ms:     the emitted blocks into device memory;
  - warp_dry_ms:     MLM_WARP_DRY, the counts alone (candidates, sort, the gather for the live predicate);
  - warp_replace_ms: MLM_WARP_REPLACE, no outputs (before every timed call the handle is put back, not timed: everything dropped, the
                     snapshot of the whole map imported from device memory);
  - comparator_ms:   export, numpy gather, crop of everything, import (the handle is put back afterwards).
Before anything is timed the comparator's result must equal the call's output byte for byte.  The comparator takes the better part of
a second on the corridor map and much longer on the crafted one: it runs 5 x --cmp-reps times on the first, --cmp-reps times on the
second and there only for the identity and the general transform (every row carries its own "reps").  Every warp row reports the bytes
the gather must move — 6 bytes read and 6 written per voxel of an emitted block, gathered twice (count, write) — and the bytes/s that
makes of the median, beside the HBM peak.
Writes one JSON document.  Usage: python tools/warp_rate.py [--reps 30] [--warmup 2] [--cmp-reps 2] [--out profiles/warp_rate.json]"""
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
from tests import warp_ref as ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
WHOLE = ([ref.KEY_MIN] * 3, [1 << 21] * 3)
MAX_BLOCKS = 16384
TRANSFORMS = {"identity": ref.make_T(), "shift": ref.make_T(None, (0.3, -0.7, 1.1)), "yaw30": ref.make_T(ref.rot(30.0)),
              "general": ref.make_T(ref.rot(30.0, 7.0, -3.0), (0.23, -0.41, 0.17))}
PLANES = ("keys", "log_odds", "occ", "infl")


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


def build(cfg):
    m = MLMap(cfg, max_blocks=MAX_BLOCKS, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    return m


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cmp-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_rate.json"))
    a = ap.parse_args()
    cfg = S1
    C, n, d = cfg.cells_per_block, cfg.subbox_n, cfg.subbox_d_xyz
    sync = torch.cuda.synchronize
    out = {"hbm_peak_GBs": HBM_PEAK_GBS, "reps": a.reps, "warmup": a.warmup, "maps": {}, "cases": {},
           "not_measured": ["frontier-mode handles", "subbox_n other than 10", "host destinations (staged)", "MLM_WARP_SEEN", "a key box",
                            "the comparator for the shift and the yaw on the crafted map"]}

    def run_map(tag, m, reps, cmp_reps, cmp_names):
        whole = m.export_blocks()
        nb = len(whole["keys"])
        out["maps"][tag].update(blocks=nb, cells=C, map_bytes=nb * (12 + 6 * C))
        snap = {k: torch.from_numpy(whole[k]).cuda() for k in PLANES}
        sync()

        def restore():
            m.crop_blocks(*WHOLE, inside=True)
            m.import_blocks((snap["keys"].data_ptr(), nb), snap["log_odds"].data_ptr(), snap["occ"].data_ptr(), snap["infl"].data_ptr())

        def comparator(T):
            t0 = time.perf_counter()
            w = ref.warp(m.export_blocks(), T, n, d)
            m.crop_blocks(*WHOLE, inside=True)
            if len(w["keys"]):
                m.import_blocks(w["keys"], w["log_odds"], w["occ"], w["infl"])
            sync()
            return (time.perf_counter() - t0) * 1e3, w

        for name, T in TRANSFORMS.items():
            E = int(m.warp_blocks(T, dry=True)["summary"][2])
            dev = {"keys": torch.empty((E, 3), dtype=torch.int32, device="cuda"), "log_odds": torch.empty((E, C), dtype=torch.float32, device="cuda"),
                   "occ": torch.empty((E, C), dtype=torch.uint8, device="cuda"), "infl": torch.empty((E, C), dtype=torch.uint8, device="cuda")}
            ptrs = {"cap": E, **{k: v.data_ptr() for k, v in dev.items()}}
            sync()
            with_cmp = name in cmp_names
            ts = {"warp_dev_ms": [], "warp_dry_ms": [], "warp_replace_ms": [], "comparator_ms": []}
            if with_cmp:  # the same blocks on both sides before anything is timed: the call's output, the handle after REPLACE, the comparator
                res = m.warp_blocks(T, out=ptrs)
                got = {k: v.cpu().numpy() for k, v in dev.items()}
                _, w = comparator(T)
                assert all(got[k].tobytes() == w[k].tobytes() for k in PLANES), "the comparator computes another map"
                after_cmp = m.export_blocks()
                restore()
                m.warp_blocks(T, replace=True)
                after = m.export_blocks()
                assert all(after[k].tobytes() == after_cmp[k].tobytes() == got[k].tobytes() for k in PLANES), "MLM_WARP_REPLACE holds another map"
                restore()
            summary = None
            for r in range(a.warmup + reps):
                for k, kw in (("warp_dev_ms", dict(out=ptrs)), ("warp_dry_ms", dict(dry=True)), ("warp_replace_ms", dict(replace=True))):
                    sync()
                    t0 = time.perf_counter()
                    res = m.warp_blocks(T, **kw)
                    sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    if k == "warp_replace_ms":
                        restore()
                    if r >= a.warmup:
                        ts[k].append(dt)
                        if k == "warp_dev_ms":
                            summary = [int(v) for v in res["summary"]]
                if with_cmp and len(ts["comparator_ms"]) < cmp_reps:  # (in the same loop; seconds per call, so fewer of them and no warm-up)
                    dt, _ = comparator(T)
                    restore()
                    ts["comparator_ms"].append(dt)
            row = {k: stats(v) for k, v in ts.items() if v}
            gather = 2 * 12 * E * C  # (6 bytes read and 6 written per voxel of an emitted block, gathered twice)
            for k in ("warp_dev_ms", "warp_dry_ms", "warp_replace_ms"):
                med = row[k]["median"]
                b = gather if k == "warp_dev_ms" else (gather // 4 if k == "warp_dry_ms" else gather + 2 * (12 + 6 * C) * E)
                row[k].update(rule_bytes=b, achieved_GBs=b / (med * 1e-3) / 1e9, fraction_of_hbm_peak=b / (med * 1e-3) / 1e9 / HBM_PEAK_GBS)
                if with_cmp:
                    row[k]["comparator_over_call"] = row["comparator_ms"]["median"] / med
            row.update(T_sd=[float(v) for v in T], summary=summary, emitted=E)
            out["cases"][f"{tag}_{name}"] = row
            print(tag, name, json.dumps({k: v["median"] for k, v in row.items() if isinstance(v, dict)}), flush=True)

    out["maps"]["corridor"] = {"config": "S1", "scene": "corridor", "frames": 64}
    m = build(cfg)
    run_map("corridor", m, a.reps, min(a.reps, 5 * a.cmp_reps), list(TRANSFORMS))
    m.close()
    out["maps"]["crafted"] = {"config": "S1", "scene": "32 x 32 x 16 block keys, random planes"}
    big = MLMap(cfg, max_blocks=2 * MAX_BLOCKS, max_batch=8)
    rng = np.random.default_rng(0)
    kx, ky, kz = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing="ij")
    keys = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.int32)[rng.permutation(MAX_BLOCKS)]
    big.import_blocks(keys, rng.uniform(-2, 4, size=(MAX_BLOCKS, C)).astype(np.float32), rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(MAX_BLOCKS, C)),
                      rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(MAX_BLOCKS, C)))
    run_map("crafted", big, max(3, a.reps // 3), a.cmp_reps, ["identity", "general"])
    big.close()
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
