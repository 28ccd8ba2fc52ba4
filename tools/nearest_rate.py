"""Rate of mlm_query_nearest, beside the only way a client has to get the number without it: mlm_export_esdf (sqdist only, the same
max_dist) over the bounding box of the same points.

The map: the synthetic corridor (2 m wide, 3 m tall), S1, one frame per metre over 41 m along a heading of --yaw degrees (a
trajectory is rarely parallel to an axis of the map; the heading decides the comparator's box and is stated with it).  The points:
equally spaced along a 40 m polyline that weaves +-0.6 m across the corridor and +-0.4 m in height — 4 096 of them (a fine
trajectory, or a few hundred control points of a dozen candidates) and 2^18 (a sampled swarm of candidates).  Device in / device
out, OCC, C = 8, 16 and 64.  Per row, median of three runs each (same process, same map), host clock around call + synchronise:
  - nearest_ms: mlm_query_nearest, all five outputs;
  - esdf_ms: mlm_export_esdf into device memory, sqdist only, over the voxel bounding box of the points (box_dims, box_voxels);
  - ratio: esdf_ms / nearest_ms (> 1: mlm_query_nearest is faster).
Worst case: C = 64 on points in the middle of 14^3 blocks of FREE space with nothing in range, so every point scans its whole 129^3
cube and answers "none": nearest_ms for 4 096 and 2^18 points, no comparator.
  - mirror_us_per_point: single-point calls at C = 8 through the host mirror (default knobs).
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel's own times.
Usage: python tools/nearest_rate.py [--yaw 30] [--out profiles/nearest_rate.json]"""
import argparse
import ctypes
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

COUNTS = (4096, 1 << 18)
CS = (8, 16, 64)
LENGTH = 40.0


def build_map(yaw):
    m = MLMap(S1, max_blocks=32768, max_batch=8)
    img = syn.corridor_depth(S1)
    q = syn.quat_from_rpy(0.0, 0.0, yaw)
    for k in range(42):
        m.update_map(img, q, np.array([k * math.cos(yaw), k * math.sin(yaw), 1.5]))
    m.sync()
    return m


def polyline(count, yaw):
    s = np.linspace(0.5, 0.5 + LENGTH, count)
    across, up = 0.6 * np.sin(s * 1.7), 1.5 + 0.4 * np.sin(s * 0.9)
    return np.ascontiguousarray(np.stack([s * math.cos(yaw) - across * math.sin(yaw), s * math.sin(yaw) + across * math.cos(yaw), up], axis=1))


def free_space(n_side=14):
    n = S1.subbox_n
    m = MLMap(S1, max_blocks=4096)
    g = np.arange(n_side, dtype=np.int32)
    keys = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    c = n ** 3
    m.import_blocks(keys, np.zeros((len(keys), c), np.float32), np.full((len(keys), c), ord("f"), np.uint8), np.full((len(keys), c), ord("u"), np.uint8),
                    np.zeros(len(keys), np.uint8))
    return m, (n_side * n / 2.0) * S1.subbox_d_xyz


def median3(fn, sync):
    fn()
    sync()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [float(t) for t in ts]


def outputs(torch, k):
    o = {"status": torch.empty(k, dtype=torch.int8, device="cuda"), "voxel": torch.empty((k, 3), dtype=torch.int32, device="cuda"),
         "delta": torch.empty((k, 3), dtype=torch.int32, device="cuda"), "sq": torch.empty(k, dtype=torch.int64, device="cuda"),
         "dist": torch.empty(k, dtype=torch.float64, device="cuda")}
    return o, {key: v.data_ptr() for key, v in o.items()}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--yaw", type=float, default=30.0, help="heading of the corridor in degrees")
    ap.add_argument("--vgprs", type=int, default=-1, help="VGPR count of k_nearest from the build's resource usage remark")
    ap.add_argument("--git", default="", help="the commit the measured tree stands on (where the tool runs outside a checkout)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    yaw = math.radians(a.yaw)
    d = S1.subbox_d_xyz
    sync = torch.cuda.synchronize
    m = build_map(yaw)
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "scene": "corridor", "frames": 42, "yaw_deg": a.yaw, "blocks": m.block_count()}, "git": a.git or git or "unknown",
           "k_nearest_vgprs": a.vgprs, "flags": 1, "polyline_m": LENGTH, "rows": [], "worst_case": []}
    for count in COUNTS:
        pts = polyline(count, yaw)
        vox = np.floor(pts / d).astype(np.int64)
        lo, dims = vox.min(0), vox.max(0) - vox.min(0) + 1
        t_in = torch.from_numpy(pts).cuda()
        o, ptr = outputs(torch, count)
        sqd = torch.empty(int(dims.prod()), dtype=torch.int32, device="cuda")
        for C in CS:
            near, near_runs = median3(lambda: m.query_nearest_dev(t_in.data_ptr(), count, C, **ptr), sync)
            st = o["status"].cpu().numpy()
            esdf, esdf_runs = median3(lambda: m.export_esdf_dev(lo, dims, C, sqdist=sqd.data_ptr()), sync)
            out["rows"].append({"points": count, "max_dist": C, "nearest_ms": near, "nearest_ms_runs": near_runs, "points_per_s": count / near * 1e3,
                                "found": int((st == 1).sum()), "none": int((st == 0).sum()), "box_dims": [int(v) for v in dims],
                                "box_voxels": int(dims.prod()), "esdf_ms": esdf, "esdf_ms_runs": esdf_runs, "ratio": esdf / near})
    # single-point calls through the host mirror
    pts = polyline(2000, yaw)
    m.query_nearest(pts[:1], 8)
    L, h = m._L, m._h
    st, dist = np.zeros(1, np.int8), np.zeros(1, np.float64)
    t0 = time.perf_counter()
    for i in range(len(pts)):
        L.mlm_query_nearest(h, ctypes.c_void_p(pts[i:i + 1].ctypes.data), 1, 8, 1, ctypes.c_void_p(st.ctypes.data), None, None, None,
                            ctypes.c_void_p(dist.ctypes.data))
    out["mirror_us_per_point"] = (time.perf_counter() - t0) / len(pts) * 1e6
    out["host_queries"] = m.frame_stats()["n_host_queries"]
    m.close()
    # the worst case: nothing in range at C = 64
    m, mid = free_space()
    rng = np.random.default_rng(0)
    for count in COUNTS:
        pts = np.ascontiguousarray(mid + rng.uniform(-0.5 * d, 0.5 * d, size=(count, 3)))
        t_in = torch.from_numpy(pts).cuda()
        o, ptr = outputs(torch, count)
        near, near_runs = median3(lambda: m.query_nearest_dev(t_in.data_ptr(), count, 64, **ptr), sync)
        assert int((o["status"] == 0).sum()) == count
        out["worst_case"].append({"points": count, "max_dist": 64, "voxels_per_point": 129 ** 3, "nearest_ms": near, "nearest_ms_runs": near_runs, "points_per_s": count / near * 1e3,
                                  "voxels_per_s": count * 129 ** 3 / near * 1e3})
    m.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
