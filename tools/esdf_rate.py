"""Rate of mlm_export_esdf, beside mlm_export_window on the same windows and a CPU transform of the same mask.

The map and windows of tools/window_rate.py: 64 frames of the S1 room stream; windows of 64^3, 200 x 200 x 40 and 512 x 512 x 64
voxels centred on it.  Obstacles: OCC (signed: OCC | SIGNED).  Each case: warm-up calls, then repeats timed with the host clock
around call + synchronise:
  - esdf_dev_ms:  mlm_export_esdf into device tensors, channels {sqdist}, {dist, grad} and signed {sqdist, dist, grad}, C in
                  {8, 16, 32};
  - esdf_host_ms: the same into host numpy arrays (C = 16 only);
  - window_odds_grad_dev_ms: mlm_export_window {odds, grad} (max_iter 5) into device tensors, the yardstick for the field;
  - cpu_baseline: numpy_separable_ms, the separable truncated transform in numpy on the window's mask grown by C (one thread), and
                  scipy_edt_ms, scipy.ndimage.distance_transform_edt of the same mask when scipy imports (untruncated).
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times.
Usage: python tools/esdf_rate.py [--reps 5] [--warmup 2] [--no-cpu]"""
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
CHANNELS = {"sqdist": ("sqdist",), "dist+grad": ("dist", "grad"), "signed": ("sqdist", "dist", "grad")}


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


def numpy_edt(mask, C):
    """the separable truncated transform (tests/esdf_ref.py::edt_separable)"""
    f = np.where(mask, 0, C * C).astype(np.uint16)
    for axis in (2, 1, 0):
        g = f.copy()
        for k in range(1, C):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(0, -k), slice(k, None)
            a, b = tuple(a), tuple(b)
            np.minimum(g[a], f[b] + np.uint16(k * k), out=g[a])
            np.minimum(g[b], f[a] + np.uint16(k * k), out=g[b])
        f = g
    return f


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
        nv = dims[0] * dims[1] * dims[2]
        shape = (dims[2], dims[1], dims[0])
        wdev = {"odds": torch.empty(shape, dtype=torch.float32, device="cuda"),
                "grad": torch.empty(shape + (3,), dtype=torch.float64, device="cuda")}
        wp = {k: v.data_ptr() for k, v in wdev.items()}
        t_win = timed(lambda: m.export_window_dev(lo, dims, 5, **wp), a.reps, a.warmup, sync)
        del wdev
        dev = {"sqdist": torch.empty(shape, dtype=torch.int32, device="cuda"), "dist": torch.empty(shape, dtype=torch.float32, device="cuda"),
               "grad": torch.empty(shape + (3,), dtype=torch.float32, device="cuda")}
        for C in (8, 16, 32):
            for name, chans in CHANNELS.items():
                signed = name == "signed"
                ptrs = {k: dev[k].data_ptr() for k in chans}
                t_dev = timed(lambda: m.export_esdf_dev(lo, dims, C, signed=signed, **ptrs), a.reps, a.warmup, sync)
                case = {"dims": list(dims), "lo": lo, "voxels": nv, "C": C, "channels": list(chans), "signed": signed,
                        "grown_voxels": int(np.prod([d + 2 * (C - 1 + ("grad" in chans)) for d in dims])),
                        "esdf_dev_ms": t_dev, "window_odds_grad_dev_ms": t_win,
                        "esdf_dev_vs_window": t_dev["median"] / t_win["median"]}
                if C == 16:
                    flags = {k: k in chans for k in ("sqdist", "dist", "grad")}
                    case["esdf_host_ms"] = timed(lambda: m.export_esdf(lo, dims, C, signed=signed, **flags), a.reps, a.warmup, sync)
                out["cases"].append(case)
        del dev
        if not a.no_cpu:
            C = 16
            glo, gd = [v - C for v in lo], [v + 2 * C for v in dims]
            w = m.export_window(glo, gd, odds=False, occ=True)
            mask = w["occ"] == 0
            t0 = time.perf_counter()
            numpy_edt(mask, C)
            cpu = {"dims": list(dims), "C": C, "numpy_separable_ms": (time.perf_counter() - t0) * 1e3}
            if ndimage is not None:
                t0 = time.perf_counter()
                ndimage.distance_transform_edt(~mask)
                cpu["scipy_edt_ms"] = (time.perf_counter() - t0) * 1e3
            out.setdefault("cpu_baseline", []).append(cpu)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
