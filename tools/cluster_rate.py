"""Rate of mlm_export_clusters, beside mlm_export_reach on the same windows and the detour it replaces: export_window into host
memory and a flood fill in numpy.

The map and windows of tools/reach_rate.py: 64 frames of the S1 room stream; windows of 200 x 200 x 40 and 512 x 512 x 64 voxels
centred on it.  Sets: the frontier at min_size 1 and 8, OCC | INFL; connectivity 26.  Each case: warm-up calls, then repeats timed
with the host clock around call + synchronise:
  - clusters_dev_ms:   mlm_export_clusters into device tensors, {labels}, {table} and {labels, table};
  - clusters_host_ms:  the same into host numpy arrays ({labels, table});
  - summary:           the call's six counters;
  - reach_dev_ms:      mlm_export_reach {steps} on the same window (OCC | INFL obstacles, the seed at the traversable voxel nearest
                       the middle), for scale;
  - baseline_ms:       export_window(occ[, infl]) of the (grown) box into host memory + tests/cluster_ref.py, one core; and
                       scipy_label_ms, scipy.ndimage.label + find_objects of the same mask where scipy imports (time only);
  - bar:               median clusters_dev_ms {labels, table} below the median baseline by more than the larger of the two min-max
                       spreads.
Plus the worst cases on crafted maps, as OCCUPIED voxels: serpentine_3d(128) (one component through every tile) and a 256^3
checkerboard at connectivity 6 (2^23 components): no bar, the cost on record.
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` (with --no-cpu) for the kernels' own times.
Usage: python tools/cluster_rate.py [--reps 5] [--warmup 2] [--no-cpu]"""
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
from tests import cluster_ref as ref  # noqa: E402

WINDOWS = [(200, 200, 40), (512, 512, 64)]
SETS = {"frontier min_size 1": (dict(frontier=True), 1), "frontier min_size 8": (dict(frontier=True), 8), "occ|infl": (dict(occ=True, infl=True), 1)}
CAP = 1 << 16


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


def host_set(m, lo, dims, f):
    if f.get("frontier"):
        w = m.export_window([v - 1 for v in lo], [v + 2 for v in dims], odds=False, occ=True)
        return ref.frontier_set(w["occ"])
    w = m.export_window(lo, dims, odds=False, occ=True, infl=True)
    return ref.class_set(w["occ"], w["infl"], f.get("occ", False), f.get("infl", False), f.get("unknown", False))


def cluster_case(m, lo, dims, f, conn, ms, a, sync, torch, host=True):
    shape = (dims[2], dims[1], dims[0])
    lab = torch.empty(shape, dtype=torch.int32, device="cuda")
    tab = torch.empty((CAP, 16), dtype=torch.int64, device="cuda")
    row = {"connectivity": conn, "min_size": ms, "clusters_dev_ms": {}}
    for name, kw in (("labels", dict(labels=lab.data_ptr())), ("table", dict(table=tab.data_ptr(), cap=CAP)),
                     ("labels+table", dict(labels=lab.data_ptr(), table=tab.data_ptr(), cap=CAP))):
        row["clusters_dev_ms"][name] = timed(lambda: m.export_clusters_dev(lo, dims, connectivity=conn, min_size=ms, **f, **kw), a.reps, a.warmup, sync)
    if host:
        row["clusters_host_ms"] = timed(lambda: m.export_clusters(lo, dims, connectivity=conn, min_size=ms, cap=CAP, **f), a.reps, a.warmup, sync)
    row["summary"] = [int(v) for v in m.export_clusters_dev(lo, dims, connectivity=conn, min_size=ms, summary=True, **f)]
    return row


def import_occupied(S, n):
    """a map whose OCCUPIED voxels are the True voxels of S ([z][y][x]) placed at the origin, FREE elsewhere in its blocks"""
    dims = list(S.shape[::-1])
    g = np.stack(np.meshgrid(*[np.arange(-(-d // n)) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    pad = np.zeros([-(-d // n) * n for d in dims[::-1]], dtype=bool)
    pad[:dims[2], :dims[1], :dims[0]] = S
    cells = pad.reshape(pad.shape[0] // n, n, pad.shape[1] // n, n, pad.shape[2] // n, n).transpose(4, 2, 0, 1, 3, 5).reshape(-1, n ** 3)
    occ = np.where(cells, ord("o"), ord("f")).astype(np.uint8)  # (rows in the order of g: x slowest, cells [cz][cy][cx])
    m = MLMap(S1, max_blocks=max(8192, 2 * len(g)))
    m.import_blocks(g.astype(np.int32), np.zeros(occ.shape, np.float32), occ, np.full(occ.shape, ord("u"), np.uint8), np.zeros(len(g), np.uint8))
    return m, dims


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
        steps = torch.empty(shape, dtype=torch.int32, device="cuda")
        w = m.export_window(lo, dims, odds=False, occ=True, infl=True)
        iz, iy, ix = np.nonzero((w["occ"] != 0) & (w["infl"] != 0))
        k = int(np.argmin((ix - dims[0] // 2) ** 2 + (iy - dims[1] // 2) ** 2 + (iz - dims[2] // 2) ** 2))
        sd = torch.tensor([[int(ix[k]) + lo[0], int(iy[k]) + lo[1], int(iz[k]) + lo[2]]], dtype=torch.int32, device="cuda")
        reach_ms = timed(lambda: m.export_reach_dev(lo, dims, sd.data_ptr(), 1, occ=True, infl=True, steps=steps.data_ptr()), a.reps, a.warmup, sync)
        for sname, (f, ms) in SETS.items():
            case = {"dims": list(dims), "lo": lo, "voxels": int(np.prod(dims)), "set": sname, "reach_dev_ms": reach_ms,
                    **cluster_case(m, lo, dims, f, 26, ms, a, sync, torch)}
            if not a.no_cpu:
                base = timed(lambda: ref.clusters(host_set(m, lo, dims, f), 26, ms, CAP, lo), a.reps, 1, lambda: None)
                dev = case["clusters_dev_ms"]["labels+table"]
                spread = max(base["max"] - base["min"], dev["max"] - dev["min"])
                case["baseline_ms"] = base
                case["bar"] = {"spread_ms": spread, "met": bool(base["median"] - dev["median"] > spread), "ratio": base["median"] / dev["median"]}
                if ndimage is not None:
                    S = host_set(m, lo, dims, f)
                    st = ndimage.generate_binary_structure(3, 3)
                    case["scipy_label_ms"] = timed(lambda: ndimage.find_objects(ndimage.label(S, structure=st)[0]), a.reps, 1, lambda: None)
            out["cases"].append(case)
        del steps
    m.close()

    out["worst"] = []
    for name, S, conn in (("serpentine_3d(128) as OCC", ~ref.serpentine_3d(128), 6), ("checkerboard 256^3 at 6", ref.checkerboard((256, 256, 256)), 6)):
        m, dims = import_occupied(S, n)
        row = cluster_case(m, [0, 0, 0], dims, dict(occ=True), conn, 1, a, sync, torch, host=False)
        assert row["summary"][0] == int(S.sum())
        out["worst"].append({"case": name, "dims": dims, "voxels": int(np.prod(dims)), **row})
        m.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
