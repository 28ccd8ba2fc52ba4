"""Rate of mlm_export_window against the batched queries over the same voxel centres.

A map of 64 frames of the S1 room stream; windows of 64^3, 200 x 200 x 40 and 512 x 512 x 64 voxels centred on it; channels {odds} and
{odds, grad} (max_iter 5).  Each case: warm-up calls, then repeats timed with the host clock around call + synchronise:
  - window_dev_ms:  mlm_export_window into device tensors (what an optimiser on the GPU wants);
  - window_host_ms: the same into host numpy arrays (device staging + copy back);
  - query_ms:       mlm_query_odds (+ mlm_query_odd_grad for {odds, grad}) on the n x 3 centres from the host, answers back to the host.
Bytes the kernels must move at the least: the outputs plus the log-odds planes of the map blocks the (haloed) window touches.
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times.
Usage: python tools/window_rate.py [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlmapping_amd import synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402

WINDOWS = [(64, 64, 64), (200, 200, 40), (512, 512, 64)]
HALO = 5  # the halo k_window_fill reads for max_iter 5 (min(max_iter, MLM_WIN_HALO))


def centres(cfg, lo, dims):
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
    v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
    g = np.floor_divide(v, n)
    return g.astype(np.float64) * (d * n) + (v - g * n).astype(np.float64) * d + d * 0.5


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    cfg = S1
    m = MLMap(cfg, max_blocks=16384, max_batch=8)
    frames = list(syn.stream(cfg, "room", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    b = m.export_blocks()
    n = cfg.subbox_n
    mid = ((b["keys"].min(0) + b["keys"].max(0) + 1) * n) // 2
    out = {"map": {"config": "S1", "frames": 64, "blocks": int(b["keys"].shape[0]), "cells_per_block": cfg.cells_per_block},
           "reps": a.reps, "warmup": a.warmup, "cases": []}
    sync = torch.cuda.synchronize
    for dims in WINDOWS:
        lo = [int(mid[i] - dims[i] // 2) for i in range(3)]
        nv = dims[0] * dims[1] * dims[2]
        shape = (dims[2], dims[1], dims[0])
        pos = centres(cfg, lo, dims)
        for chans in (("odds",), ("odds", "grad")):
            grad = "grad" in chans
            h = HALO if grad else 0
            lo_g = np.floor_divide(np.array(lo) - h, n)
            hi_g = np.floor_divide(np.array(lo) + np.array(dims) + h - 1, n)
            touched = int(((b["keys"] >= lo_g) & (b["keys"] <= hi_g)).all(axis=1).sum())
            bytes_out = nv * (4 + (24 if grad else 0))
            bytes_planes = touched * cfg.cells_per_block * 4
            dev = {"odds": torch.empty(shape, dtype=torch.float32, device="cuda")}
            if grad:
                dev["grad"] = torch.empty(shape + (3,), dtype=torch.float64, device="cuda")
            ptrs = {k: v.data_ptr() for k, v in dev.items()}
            t_dev = timed(lambda: m.export_window_dev(lo, dims, 5, **ptrs), a.reps, a.warmup, sync)
            t_host = timed(lambda: m.export_window(lo, dims, odds=True, grad=grad, max_iter=5), a.reps, a.warmup, sync)

            def queries():
                m.getOdd(pos)
                if grad:
                    m.getOddGrad(pos, 5)

            t_q = timed(queries, a.reps, a.warmup, sync)
            out["cases"].append({
                "dims": list(dims), "lo": lo, "voxels": nv, "channels": list(chans), "max_iter": 5, "touched_blocks": touched,
                "bytes_out": bytes_out, "bytes_planes": bytes_planes,
                "window_dev_ms": t_dev, "window_host_ms": t_host, "query_ms": t_q,
                "speedup_dev_vs_query": t_q["median"] / t_dev["median"],
                "window_dev_GBps": (bytes_out + bytes_planes) / (t_dev["median"] * 1e-3) / 1e9,
            })
            del dev
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
