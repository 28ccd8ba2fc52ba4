"""Rate of mlm_export_reach, beside mlm_export_esdf on the same windows and the detour it replaces: export_window into host memory
and a breadth-first search in numpy.

The map and windows of tools/esdf_rate.py: 64 frames of the S1 room stream; windows of 200 x 200 x 40 and 512 x 512 x 64 voxels
centred on it.  Flag sets OCC | INFL and OCC | UNKNOWN, the seed at the traversable voxel nearest the window's middle, clearance 0
and 3.  Each case: warm-up calls, then repeats timed with the host clock around call + synchronise:
  - reach_dev_ms:        mlm_export_reach into device tensors, {steps} and {steps, parent};
  - reach_host_ms:       the same into host numpy arrays ({steps});
  - sweeps:              relaxation sweeps the call needed (summary[3]);
  - esdf_sqdist_dev_ms:  mlm_export_esdf {sqdist} at C = 16 into a device tensor, the yardstick for "one pass over the box";
  - baseline_ms:         (clearance 0) export_window(occ, infl) into host memory + the search of tests/reach_ref.py, one core; and
                         scipy_label_ms, scipy.ndimage.label of the same mask where scipy imports (components, no distances);
  - bar:                 median reach_dev_ms {steps} below the median baseline by more than the larger of the two min-max spreads.
Plus a crafted 512 x 512 x 8 serpentine (a wall in every other row, gaps at alternating ends) as the many-sweeps case, at
reach_group 8 (the default) and 64: no bar, the cost per sweep on record.
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` (with --no-cpu) for the kernels' own times.
Usage: python tools/reach_rate.py [--reps 5] [--warmup 2] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlmapping_amd import mlmap, synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402
from tests import reach_ref as ref  # noqa: E402

WINDOWS = [(200, 200, 40), (512, 512, 64)]
FLAGS = {"occ|infl": dict(occ=True, infl=True, unknown=False), "occ|unknown": dict(occ=True, infl=False, unknown=True)}


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


def obstacle_mask(w, f):
    m = np.zeros(w["occ"].shape, dtype=bool)
    if f["occ"]:
        m |= w["occ"] == 0
    if f["infl"]:
        m |= w["infl"] == 0
    if f["unknown"]:
        m |= w["occ"] == -1
    return m


def nearest_free(T, at):
    iz, iy, ix = np.nonzero(T)
    k = int(np.argmin((ix - at[0]) ** 2 + (iy - at[1]) ** 2 + (iz - at[2]) ** 2))
    return [int(ix[k]), int(iy[k]), int(iz[k])]


def reach_cases(m, lo, dims, f, seed, clearances, a, sync, torch):
    shape = (dims[2], dims[1], dims[0])
    dev = {"steps": torch.empty(shape, dtype=torch.int32, device="cuda"), "parent": torch.empty(shape, dtype=torch.uint8, device="cuda")}
    sd = torch.tensor([seed], dtype=torch.int32, device="cuda")
    rows = []
    for r in clearances:
        row = {"clearance": r, "reach_dev_ms": {}}
        for name, chans in (("steps", ("steps",)), ("steps+parent", ("steps", "parent"))):
            ptrs = {k: dev[k].data_ptr() for k in chans}
            row["reach_dev_ms"][name] = timed(lambda: m.export_reach_dev(lo, dims, sd.data_ptr(), 1, clearance=r, **f, **ptrs), a.reps, a.warmup, sync)
        row["reach_host_ms"] = timed(lambda: m.export_reach(lo, dims, [seed], clearance=r, **f), a.reps, a.warmup, sync)
        sm = m.export_reach_dev(lo, dims, sd.data_ptr(), 1, clearance=r, summary=True, **f)
        row.update(traversable=int(sm[0]), reached=int(sm[1]), largest_steps=int(sm[2]), sweeps=int(sm[3]))
        rows.append(row)
    return rows


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy / scipy baselines (profiling runs)")
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
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    out = {"map": {"config": "S1", "frames": 64, "blocks": int(b["keys"].shape[0])}, "reps": a.reps, "warmup": a.warmup,
           "scipy": ndimage is not None, "cases": []}
    sync = torch.cuda.synchronize
    for dims in WINDOWS:
        lo = [int(mid[i] - dims[i] // 2) for i in range(3)]
        shape = (dims[2], dims[1], dims[0])
        sq = torch.empty(shape, dtype=torch.int32, device="cuda")
        w = m.export_window(lo, dims, odds=False, occ=True, infl=True)
        for fname, f in FLAGS.items():
            T = ~obstacle_mask(w, f)
            rel_seed = nearest_free(T, [d // 2 for d in dims])
            seed = [rel_seed[i] + lo[i] for i in range(3)]
            case = {"dims": list(dims), "lo": lo, "voxels": int(np.prod(dims)), "flags": fname, "seed": seed,
                    "esdf_sqdist_dev_ms": timed(lambda: m.export_esdf_dev(lo, dims, 16, sqdist=sq.data_ptr(), **f), a.reps, a.warmup, sync),
                    "reach": reach_cases(m, lo, dims, f, seed, (0, 3), a, sync, torch)}
            if not a.no_cpu:
                def detour():
                    ww = m.export_window(lo, dims, odds=False, occ=True, infl=True)
                    return ref.reach(~obstacle_mask(ww, f), [rel_seed])

                base = timed(detour, a.reps, 1, lambda: None)
                dev = case["reach"][0]["reach_dev_ms"]["steps"]
                spread = max(base["max"] - base["min"], dev["max"] - dev["min"])
                case["baseline_ms"] = base
                case["bar"] = {"spread_ms": spread, "met": bool(base["median"] - dev["median"] > spread), "ratio": base["median"] / dev["median"]}
                if ndimage is not None:
                    case["scipy_label_ms"] = timed(lambda: ndimage.label(T), a.reps, 1, lambda: None)
            out["cases"].append(case)
        del sq
    m.close()

    # the many-sweeps case: a serpentine slab imported voxel by voxel
    dims, lo = [512, 512, 8], [0, 0, 0]
    blocked = ref.serpentine_slab(dims[0], dims[1], dims[2])
    g = np.stack(np.meshgrid(*[np.arange(-(-d // n)) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    pad = np.zeros([-(-d // n) * n for d in dims[::-1]], dtype=bool)
    pad[:dims[2], :dims[1], :dims[0]] = blocked
    cells = pad.reshape(pad.shape[0] // n, n, pad.shape[1] // n, n, pad.shape[2] // n, n).transpose(4, 2, 0, 1, 3, 5).reshape(-1, n ** 3)
    occ = np.where(cells, ord("o"), ord("f")).astype(np.uint8)  # (rows in the order of g: x slowest, cells [cz][cy][cx])
    m = MLMap(cfg, max_blocks=8192)
    m.import_blocks(g.astype(np.int32), np.zeros(occ.shape, np.float32), occ, np.full(occ.shape, ord("u"), np.uint8), np.zeros(len(g), np.uint8))
    f = dict(occ=True, infl=False, unknown=False)
    w = m.export_window(lo, dims, odds=False, occ=True)
    assert np.array_equal(w["occ"] == 0, blocked)
    serp = {"dims": dims, "voxels": int(np.prod(dims)), "groups": {}}
    try:
        for group in (8, 64):
            mlmap.debug_set("reach_group", group)
            serp["groups"][str(group)] = reach_cases(m, lo, dims, f, [0, 0, 0], (0,), a, sync, torch)[0]
    finally:
        mlmap.load_library().mlm_debug_reset()
    out["serpentine"] = serp
    m.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
