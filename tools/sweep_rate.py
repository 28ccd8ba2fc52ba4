"""Rate of mlm_query_sweeps, beside its floor and beside what a client does today without it.

The map: the synthetic corridor (2 m wide, 3 m tall), S1, one frame per metre over 64 frames along a heading of --yaw degrees.  The
edges: tools/ray_rate.py's "edges" batch — both end points uniform in the map's bounding box — 2^16 and 2^20 of them, device in / device
out, all seven outputs, OCC, radius 0, 1, 2, 4, 8 and 16.  Per row, median of 30 calls each (same process, same map, one loop), host
clock around call + synchronise:
  - sweeps_ms: mlm_query_sweeps;
  - rays_ms: (a) mlm_query_rays on the same edges, OCC, all five outputs — the floor; radius 0 should land within noise of it;
  - today_ms: (b) mlm_export_esdf {sqdist} at max_dist r + 1 over the voxel bounding box of the batch (esdf_ms), plus mlm_query_rays
    with flags 0 for the path lengths (rays0_ms), plus one torch gather of sqdist at the end voxels (gather_ms) as the lower bound of
    the rest — the gather along every path that the caller still has to write is not in it.  A box of more than 2^31 - 1 voxels cannot
    be exported in one call: box_too_large, and no today_ms;
  - ratio: today_ms / sweeps_ms (> 1: mlm_query_sweeps is faster);
  - columns, passes: L(r) and the 64-lane passes per step, ceil(L(r) / 64) (radius 0 runs a lane per ray); lane_use: L(r) / (64 passes).
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times.
Usage: python tools/sweep_rate.py [--yaw 30] [--calls 30] [--out profiles/sweep_rate.json]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd import synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402

COUNTS = (1 << 16, 1 << 20)
RADII = (0, 1, 2, 4, 8, 16)
FRAMES = 64


def build_map(yaw):
    m = MLMap(S1, max_blocks=65536, max_batch=8)
    img = syn.corridor_depth(S1)
    q = syn.quat_from_rpy(0.0, 0.0, yaw)
    for k in range(FRAMES):
        m.update_map(img, q, np.array([k * math.cos(yaw), k * math.sin(yaw), 1.5]))
    m.sync()
    return m


def columns(r):
    return sum(1 for p in range(-r, r + 1) for q in range(-r, r + 1) if p * p + q * q <= r * r)


def median_of(fn, sync, calls):
    fn()
    sync()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--yaw", type=float, default=30.0, help="heading of the corridor in degrees")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--git", default="", help="the commit the measured tree stands on (where the tool runs outside a checkout)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    yaw = math.radians(a.yaw)
    d, n = S1.subbox_d_xyz, S1.subbox_n
    sync = torch.cuda.synchronize
    m = build_map(yaw)
    b = m.export_blocks()
    lo_w, hi_w = b["keys"].min(0) * d * n, (b["keys"].max(0) + 1) * d * n
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "scene": "corridor", "frames": FRAMES, "yaw_deg": a.yaw, "blocks": int(b["keys"].shape[0])}, "git": a.git or git or "unknown",
           "flags": 1, "calls": a.calls, "rows": []}
    rng = np.random.default_rng(0)
    for count in COUNTS:
        p0, p1 = rng.uniform(lo_w, hi_w, size=(count, 3)), rng.uniform(lo_w, hi_w, size=(count, 3))
        t0, t1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
        o = {"status": torch.empty(count, dtype=torch.int8, device="cuda"), "voxel": i32(count, 3), "t": torch.empty(count, dtype=torch.float64, device="cuda"),
             "n_steps": i32(count), "n_unknown": i32(count), "hit": i32(count, 3), "hit_sq": i32(count)}
        ray_ptr = {k: o[k].data_ptr() for k in ("status", "voxel", "t", "n_steps", "n_unknown")}
        L, h = m._L, m._h
        import ctypes
        vp = ctypes.c_void_p
        outs = [vp(o[k].data_ptr()) for k in ("status", "voxel", "t", "n_steps", "n_unknown", "hit", "hit_sq")]
        vox = np.floor(np.concatenate([p0, p1]) / d).astype(np.int64)
        blo, dims = vox.min(0), vox.max(0) - vox.min(0) + 1
        box_voxels = int(dims.prod())
        rays = median_of(lambda: m.cast_rays_dev(t0.data_ptr(), t1.data_ptr(), count, occ=True, **ray_ptr), sync, a.calls)
        rays0 = median_of(lambda: m.cast_rays_dev(t0.data_ptr(), t1.data_ptr(), count, occ=False, **ray_ptr), sync, a.calls)
        path_voxels = int(o["n_steps"].to(torch.int64).sum())  # (flags 0: N + 1 per valid ray)
        sqd = torch.empty(box_voxels, dtype=torch.int32, device="cuda") if box_voxels <= 2 ** 31 - 1 else None
        tlo = torch.from_numpy(blo).cuda()
        tdims = torch.from_numpy(dims).cuda()

        def gather():
            v = o["voxel"].to(torch.int64) - tlo
            return sqd[(v[:, 2] * tdims[1] + v[:, 1]) * tdims[0] + v[:, 0]]

        for r in RADII:
            sw = median_of(lambda: L.mlm_query_sweeps(h, vp(t0.data_ptr()), vp(t1.data_ptr()), count, r, 1, *outs), sync, a.calls)
            st = o["status"].cpu().numpy()
            cols = columns(r)
            passes = (cols + 63) // 64
            row = {"edges": count, "radius": r, "columns": cols, "passes": passes if r else 0, "lane_use": cols / (64.0 * passes) if r else 1.0,
                   "sweeps_ms": sw[0], "sweeps_ms_min_max": sw[1:], "edges_per_s": count / sw[0] * 1e3, "stopped": int((st == 1).sum()),
                   "not_stopped": int((st == 0).sum()), "stopped_at_start": int(((st == 1) & (o["n_steps"].cpu().numpy() == 0)).sum()),
                   "rays_ms": rays[0], "rays_ms_min_max": rays[1:], "over_floor": sw[0] / rays[0], "path_voxels": path_voxels,
                   "box_dims": [int(v) for v in dims], "box_voxels": box_voxels}
            if sqd is None:
                row["box_too_large"] = True
            else:
                esdf = median_of(lambda: m.export_esdf_dev(blo, dims, r + 1, sqdist=sqd.data_ptr()), sync, a.calls)
                m.cast_rays_dev(t0.data_ptr(), t1.data_ptr(), count, occ=False, **ray_ptr)  # (the end voxels the gather reads)
                g = median_of(gather, sync, a.calls)
                row.update({"esdf_ms": esdf[0], "esdf_ms_min_max": esdf[1:], "rays0_ms": rays0[0], "gather_ms": g[0], "today_ms": esdf[0] + rays0[0] + g[0],
                            "ratio": (esdf[0] + rays0[0] + g[0]) / sw[0]})
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    m.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
