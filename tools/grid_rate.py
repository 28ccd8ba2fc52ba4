"""Rate of mlm_export_grid2d against the detour without it: mlm_export_window of the whole slab plus a reduction along z in torch.

The map of tools/window_rate.py (64 frames of the S1 room stream); slabs of 512 x 512 x 64 voxels and a thin band of 2048 x 2048 x 8
centred on it.  Per slab, everything into device memory, on one stream, timed with events on that stream (warm-up calls, then the
median over the repeats; the host clock around call + synchronise is recorded beside it):
  - grid_ms:        export_grid2d {grid}
  - grid_cols_ms:   export_grid2d {grid, cols}
  - grid_dist_ms:   export_grid2d {grid, sqdist, dist} at C = 16
  - window_ms:      export_window {occ, infl} of the same box — the detour's first half, which writes dims[2] times the cells
  - reduce_ms:      the detour's second half in torch: n_obs / n_unk / n_free, lowest and highest occupied z and the grid along z
The expectation: grid_cols_ms <= window_ms (same planes read, about 1 / dims[2] of the bytes written); both and their ratio are in
the JSON, as are the detour's grid and counts compared with export_grid2d's.
Prints one JSON document.  Usage: python tools/grid_rate.py [--reps 20] [--warmup 3]"""
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

SLABS = [(512, 512, 64), (2048, 2048, 8)]
C = 16


def timed(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {"median": float(np.median(ev)), "min": float(np.min(ev)), "max": float(np.max(ev)), "host_median": float(np.median(host))}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfg = S1
    m = MLMap(cfg, max_blocks=16384, max_batch=8)
    frames = list(syn.stream(cfg, "room", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)  # (the events are recorded on the stream the kernels run on)
    b = m.export_blocks()
    n = cfg.subbox_n
    mid = ((b["keys"].min(0) + b["keys"].max(0) + 1) * n) // 2
    out = {"status": "measured", "device": torch.cuda.get_device_name(0),
           "map": {"config": "S1", "frames": 64, "blocks": int(b["keys"].shape[0]), "cells_per_block": cfg.cells_per_block},
           "reps": a.reps, "warmup": a.warmup, "max_dist": C, "cases": []}
    torch.cuda.set_stream(stream)
    for dims in SLABS:
        lo = [int(mid[i] - dims[i] // 2) for i in range(3)]
        plane, vol = (dims[1], dims[0]), (dims[2], dims[1], dims[0])
        g = torch.empty(plane, dtype=torch.int8, device="cuda")
        cols = torch.empty(plane + (8,), dtype=torch.int32, device="cuda")
        sq = torch.empty(plane, dtype=torch.int32, device="cuda")
        di = torch.empty(plane, dtype=torch.float32, device="cuda")
        occ = torch.empty(vol, dtype=torch.int8, device="cuda")
        infl = torch.empty(vol, dtype=torch.int8, device="cuda")
        z = (lo[2] + torch.arange(dims[2], device="cuda", dtype=torch.int32))[:, None, None]
        red = {}

        def reduce():
            o = occ == 0
            red["n_obs"], red["n_unk"], red["n_free"] = o.sum(0, dtype=torch.int32), (occ == -1).sum(0, dtype=torch.int32), (occ == 1).sum(0, dtype=torch.int32)
            red["zmin"] = torch.where(o, z, lo[2] + dims[2]).amin(0)
            red["zmax"] = torch.where(o, z, lo[2] - 1).amax(0)
            red["grid"] = torch.where(red["n_obs"] > 0, 100, 0).to(torch.int8)

        t_grid = timed(lambda: m.export_grid2d_dev(lo, dims, grid=g.data_ptr()), a.reps, a.warmup)
        t_dist = timed(lambda: m.export_grid2d_dev(lo, dims, max_dist=C, grid=g.data_ptr(), sqdist=sq.data_ptr(), dist=di.data_ptr()), a.reps, a.warmup)
        t_cols = timed(lambda: m.export_grid2d_dev(lo, dims, grid=g.data_ptr(), cols=cols.data_ptr()), a.reps, a.warmup)
        t_win = timed(lambda: m.export_window_dev(lo, dims, 0, occ=occ.data_ptr(), infl=infl.data_ptr()), a.reps, a.warmup)
        t_red = timed(reduce, a.reps, a.warmup)
        same = bool(torch.equal(red["grid"], g) and torch.equal(red["n_obs"], cols[..., 0]) and torch.equal(red["n_unk"], cols[..., 1])
                    and torch.equal(red["n_free"], cols[..., 2]) and torch.equal(red["zmin"], cols[..., 3]) and torch.equal(red["zmax"], cols[..., 4]))
        cells, vox = dims[0] * dims[1], dims[0] * dims[1] * dims[2]
        out["cases"].append({
            "dims": list(dims), "lo": lo, "cells": cells, "voxels": vox, "occupied_cells": int((g == 100).sum()),
            "bytes_written_grid_cols": cells * 33, "bytes_written_window": vox * 2,
            "grid_ms": t_grid, "grid_cols_ms": t_cols, "grid_dist_ms": t_dist, "window_ms": t_win, "reduce_ms": t_red,
            "grid_cols_over_window": t_cols["median"] / t_win["median"],
            "grid_cols_no_slower_than_window": bool(t_cols["median"] <= t_win["median"]),
            "detour_over_grid_cols": (t_win["median"] + t_red["median"]) / t_cols["median"],
            "detour_agrees": same,
        })
        del g, cols, sq, di, occ, infl
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
