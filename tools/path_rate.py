"""Rate of mlm_query_paths beside the cheapest thing a caller could do without it: copying the parent field to the host.

The map: 64 frames of the S1 corridor stream.  The field: mlm_export_route over 512 x 512 x 64 voxels centred on the vehicle
(connectivity 26, clearance 1, penalties (30, 10, 3), obstacles OCC, seeds the 27 voxels round the vehicle), its parent bytes in a
device tensor.  The goals, in a device tensor: the root voxels of mlm_export_clusters' frontier components of that box (at most
4 096) and 4 096 random reached voxels.  Per lookahead in (16, 64, 256), device in, device out (status, way with cap 64, length,
table), max_moves the binding's default:
  paths_ms:  warm-up calls, then repeats timed with the host clock around call + synchronise (median, min, max);
  copy_ms:   the device-to-host copy of the parent field alone (16 MiB) into pinned host memory, timed the same way in the same loop,
             the two alternating — a lower bound for every host-side walk, which would still have to chase the codes and shorten;
  copy_pageable_ms: the same copy into pageable memory (tensor.cpu()).
Fixes no ratio: both times go into the JSON; slower_than_copy says where the call loses.  Also the goals' statuses, the mean moves
and way points, and the candidates tested beyond the chosen ones (table word 6).
Prints one JSON document.  Usage: python tools/path_rate.py [--reps 30] [--warmup 3]"""
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

DIMS = (512, 512, 64)
ROUTE = dict(occ=True, infl=False, unknown=False, clearance=1, connectivity=26, move_cost=(10, 14, 17), penalty=(30, 10, 3))
LOOKAHEADS = (16, 64, 256)


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfg = S1
    m = MLMap(cfg, max_blocks=16384, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    vehicle = np.array([int(np.floor(v / cfg.subbox_d_xyz)) for v in frames[-1][1][1]])
    dims = list(DIMS)
    lo = [int(vehicle[i] - dims[i] // 2) for i in range(3)]
    sync = torch.cuda.synchronize
    off = np.array([(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)])
    seeds = torch.from_numpy((vehicle + off).astype(np.int32)).cuda()
    field = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.uint8, device="cuda")
    t0 = time.perf_counter()
    summary = m.export_route_dev(lo, dims, seeds.data_ptr(), 27, parent=field.data_ptr(), summary=True, **ROUTE)
    sync()
    route_ms = (time.perf_counter() - t0) * 1e3
    parent = field.cpu().numpy()
    reached = np.argwhere(parent <= 26)[:, ::-1]
    rng = np.random.default_rng(7)
    random_goals = reached[rng.choice(len(reached), size=min(4096, len(reached)), replace=False)] + np.asarray(lo)
    roots = m.export_clusters(lo, dims, frontier=True, labels=False, cap=4096)["table"][:, 1:4]
    goals = torch.from_numpy(np.ascontiguousarray(np.concatenate([roots, random_goals]).astype(np.int32))).cuda()
    pinned = torch.empty(field.shape, dtype=torch.uint8, pin_memory=True)
    rows = {}
    for L in LOOKAHEADS:
        def paths():
            return m.query_paths(lo, dims, field, goals, "route", L, None, 64)

        def copy():
            pinned.copy_(field, non_blocking=True)

        for _ in range(a.warmup):
            paths()
            copy()
            field.cpu()
        sync()
        tp, tc, tg = [], [], []
        for _ in range(a.reps):
            for fn, ts in ((paths, tp), (copy, tc), (lambda: field.cpu(), tg)):
                t0 = time.perf_counter()
                fn()
                sync()
                ts.append((time.perf_counter() - t0) * 1e3)
        out = {k: v.cpu().numpy() for k, v in paths().items()}
        ok = out["status"] == 1
        rows[str(L)] = {"paths_ms": stats(tp), "copy_ms": stats(tc), "copy_pageable_ms": stats(tg),
                        "slower_than_copy": bool(np.median(tp) > np.median(tc)),
                        "status": {str(s): int((out["status"] == s).sum()) for s in (1, 0, -1, -2)},
                        "mean_moves": float(out["table"][ok, 0].mean()) if ok.any() else 0.0,
                        "mean_waypoints": float(out["table"][ok, 1].mean()) if ok.any() else 0.0,
                        "longest_path": int(out["table"][:, 0].max()), "candidates_beyond": int(out["table"][ok, 6].sum())}
    doc = {"map": {"config": "S1", "scene": "corridor", "frames": 64}, "dims": dims, "lo": lo, "voxels": int(np.prod(dims)),
           "field_bytes": int(field.numel()), "route": {k: list(v) if isinstance(v, tuple) else v for k, v in ROUTE.items()},
           "route_summary": [int(v) for v in summary], "route_first_call_ms": route_ms, "goals": int(goals.shape[0]),
           "frontier_roots": int(len(roots)), "max_moves": MLMap._path_max_moves(dims, None), "cap": 64, "reps": a.reps, "warmup": a.warmup,
           "rows": rows}
    m.close()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
