"""Rate of mlm_export_route beside mlm_export_reach on the same window, and the numpy reference on one core.

The map and the large window of tools/reach_rate.py: 64 frames of the S1 room stream, 512 x 512 x 64 voxels centred on it, flags
OCC | INFL, the seed at the traversable voxel nearest the window's middle, device seeds and device outputs ({steps} / {cost}).
Each row: warm-up calls, then repeats timed with the host clock around call + synchronise (median, min, max), and the
relaxation sweeps the call needed (summary[3]):
  (a) reach:        mlm_export_reach, clearance 0;
  (b) route6:       mlm_export_route at connectivity 6, move_cost 1, no penalty (the same field as (a));
  (c) route26:      mlm_export_route at connectivity 26, move_cost (10, 14, 17);
  (d) route26_pen:  mlm_export_route at connectivity 26, clearance 1, penalty (30, 10, 3).
ratio_b_over_a: the medians' ratio.  numpy_ref: tests/route_ref.py's route() at connectivity 26 with the penalties of (d) on a
61 x 47 x 17 window round the middle, one core.
Prints one JSON document.  Usage: python tools/route_rate.py [--reps 7] [--warmup 3] [--no-cpu]"""
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
from tests import route_ref as ref  # noqa: E402

DIMS = (512, 512, 64)
FLAGS = dict(occ=True, infl=True, unknown=False)


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


def obstacle_mask(w):
    return (w["occ"] == 0) | (w["infl"] == 0)


def nearest_free(T, at):
    iz, iy, ix = np.nonzero(T)
    k = int(np.argmin((ix - at[0]) ** 2 + (iy - at[1]) ** 2 + (iz - at[2]) ** 2))
    return [int(ix[k]), int(iy[k]), int(iz[k])]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy reference")
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
    dims = list(DIMS)
    lo = [int(mid[i] - dims[i] // 2) for i in range(3)]
    shape = (dims[2], dims[1], dims[0])
    sync = torch.cuda.synchronize
    w = m.export_window(lo, dims, odds=False, occ=True, infl=True)
    rel_seed = nearest_free(~obstacle_mask(w), [d // 2 for d in dims])
    seed = [rel_seed[i] + lo[i] for i in range(3)]
    out_dev = torch.empty(shape, dtype=torch.int32, device="cuda")
    sd = torch.tensor([seed], dtype=torch.int32, device="cuda")
    rows = {}

    def row(name, call, **kw):
        ms = timed(lambda: call(lo, dims, sd.data_ptr(), 1, **FLAGS, **kw, **{("steps" if name == "reach" else "cost"): out_dev.data_ptr()}),
                   a.reps, a.warmup, sync)
        sm = call(lo, dims, sd.data_ptr(), 1, summary=True, **FLAGS, **kw)
        rows[name] = {"args": {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}, "ms": ms, "traversable": int(sm[0]),
                      "reached": int(sm[1]), "largest": int(sm[2]), "sweeps": int(sm[3])}

    row("reach", m.export_reach_dev, clearance=0)
    row("route6", m.export_route_dev, clearance=0, connectivity=6, move_cost=(1, 1, 1))
    row("route26", m.export_route_dev, clearance=0, connectivity=26, move_cost=(10, 14, 17))
    row("route26_pen", m.export_route_dev, clearance=1, connectivity=26, move_cost=(10, 14, 17), penalty=(30, 10, 3))
    out = {"map": {"config": "S1", "frames": 64, "blocks": int(b["keys"].shape[0])}, "dims": dims, "lo": lo, "voxels": int(np.prod(dims)),
           "flags": "occ|infl", "seed": seed, "reps": a.reps, "warmup": a.warmup, "rows": rows,
           "ratio_b_over_a": rows["route6"]["ms"]["median"] / rows["reach"]["ms"]["median"]}
    if not a.no_cpu:
        sdims, r, pen = [61, 47, 17], 1, (30, 10, 3)
        slo = [int(mid[i] - sdims[i] // 2) for i in range(3)]
        g = r + len(pen) + 1
        ww = m.export_window([v - g for v in slo], [v + 2 * g for v in sdims], odds=False, occ=True, infl=True)
        cls = ref.classes(obstacle_mask(ww), r, len(pen))
        s = nearest_free(cls != ref.BLOCKED, [d // 2 for d in sdims])
        t0 = time.perf_counter()
        exp = ref.route(cls, [s], 26, (10, 14, 17), pen)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = m.export_route(slo, sdims, [[s[i] + slo[i] for i in range(3)]], clearance=r, penalty=pen, **FLAGS)
        dev_ms = timed(lambda: m.export_route(slo, sdims, [[s[i] + slo[i] for i in range(3)]], clearance=r, penalty=pen, **FLAGS), a.reps, a.warmup, sync)
        out["numpy_ref"] = {"dims": sdims, "voxels": int(np.prod(sdims)), "reached": int(exp["summary"][1]), "ms": cpu_ms,
                            "route_host_ms": dev_ms, "equal": bool(np.array_equal(got["cost"], exp["cost"]))}
    m.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
