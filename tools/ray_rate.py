"""Rate of mlm_query_rays, beside the only alternative a client has without it: the voxel centres of the same paths through
mlm_query_occupancy + mlm_query_inflate_occupancy.

The map: S1 after 48 room_jitter frames (inflate_map twice).  Two batches of 2^20 rays, device in / device out:
  - edges: both end points uniform in the map's bounding box, OCC | INFL (a sampling planner's collision checks);
  - views: 4 096 origins in free space x 256 directions, 8 m long, OCC (an exploration planner's view scoring, n_unknown).
Per batch, median of three runs each (same process, same map), host clock around call + synchronise:
  - rays_ms: mlm_query_rays (all five outputs), rays/s and voxels visited/s (from n_steps);
  - yardstick_ms: the centres of the voxels the rays visited (enumerated on the host beforehand, not timed) through one
    mlm_query_occupancy + one mlm_query_inflate_occupancy call per 2^24 centres, knob "mirror" = 0 — the upload of the centres
    is part of it: that is what the client pays.  Enumerating every visited voxel takes host memory (24 bytes each), so the
    yardstick runs on the first --yard-rays rays of the batch and is scaled by voxels; the ratio compares time per voxel.
  - mirror_us_per_ray: single-ray calls of the edges batch through the host mirror (default knobs).
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel's own times.
Usage: python tools/ray_rate.py [--yard-rays 65536] [--out profiles/ray_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd import mlmap, synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402

N_RAYS = 1 << 20
OCC, INFL = 1, 2


def build_map():
    m = MLMap(S1, max_blocks=16384, max_batch=8)
    frames = list(syn.stream(S1, "room_jitter", "smooth", 48))
    for k0 in range(0, 48, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
        m.inflate_map(fr[-1][1][1])
    m.sync()
    return m


def visited_centres(p0, p1, n_steps, cfg):
    """centres of the first n_steps voxels of every ray's path (the walk of include/mlmap_hip.h, vectorised over the rays)"""
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    Q0 = np.floor((p0 / d) * 1024.0).astype(np.int64)
    Q1 = np.floor((p1 / d) * 1024.0).astype(np.int64)
    Dq = Q1 - Q0
    s, ad = np.sign(Dq), np.abs(Dq)
    v = Q0 >> 10
    e = Q1 >> 10
    m = np.where(s > 0, ((v + 1) << 10) - Q0, Q0 - (v << 10)) * (s != 0)
    out = []
    alive = np.arange(len(p0))
    k = 0
    while alive.size:
        alive = alive[n_steps[alive] > k]
        if not alive.size:
            break
        out.append(v[alive].copy())
        go = v[alive] != e[alive]
        best = np.full(alive.size, -1)
        bm, bd = np.zeros(alive.size, np.int64), np.ones(alive.size, np.int64)
        for a in range(3):
            take = go[:, a] & ((best < 0) | (m[alive, a] * bd < bm * ad[alive, a]))
            best[take] = a
            bm[take] = m[alive, a][take]
            bd[take] = ad[alive, a][take]
        mv = best >= 0
        v[alive[mv], best[mv]] += s[alive[mv], best[mv]]
        m[alive[mv], best[mv]] += 1024
        k += 1
    vox = np.concatenate(out)
    g = np.floor_divide(vox, n)
    return g.astype(np.float64) * (d * n) + (vox - g * n).astype(np.float64) * d + d * 0.5


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


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--yard-rays", type=int, default=65536)
    ap.add_argument("--vgprs", type=int, default=-1, help="VGPR count of k_rays from the build's resource usage remark")
    ap.add_argument("--git", default="", help="the commit the measured tree stands on (where the tool runs outside a checkout)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = S1
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    m = build_map()
    b = m.export_blocks()
    lo, hi = b["keys"].min(0) * d * n, (b["keys"].max(0) + 1) * d * n
    rng = np.random.default_rng(0)
    batches = {}
    batches["edges"] = (rng.uniform(lo, hi, size=(N_RAYS, 3)), rng.uniform(lo, hi, size=(N_RAYS, 3)), OCC | INFL)
    cand = rng.uniform(lo, hi, size=(200000, 3))
    org = cand[m.getOccupancy(cand) == 1][:4096]
    assert len(org) == 4096, len(org)
    u = rng.normal(size=(4096, 256, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    batches["views"] = (np.repeat(org, 256, axis=0), (org[:, None, :] + 8.0 * u).reshape(-1, 3), OCC)
    sync = torch.cuda.synchronize
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "frames": 48, "blocks": int(b["keys"].shape[0])}, "rays": N_RAYS, "git": a.git or git or "unknown",
           "k_rays_vgprs": a.vgprs, "batches": {}}

    def dev_case(mm, p0, p1, flags):
        t0, t1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
        o = {"status": torch.empty(N_RAYS, dtype=torch.int8, device="cuda"), "voxel": torch.empty((N_RAYS, 3), dtype=torch.int32, device="cuda"),
             "t": torch.empty(N_RAYS, dtype=torch.float64, device="cuda"), "n_steps": torch.empty(N_RAYS, dtype=torch.int32, device="cuda"),
             "n_unknown": torch.empty(N_RAYS, dtype=torch.int32, device="cuda")}
        ptr = {k: v.data_ptr() for k, v in o.items()}
        med, runs = median3(lambda: mm.cast_rays_dev(t0.data_ptr(), t1.data_ptr(), N_RAYS, occ=bool(flags & OCC), infl=bool(flags & INFL), **ptr), sync)
        return med, runs, {k: v.cpu().numpy() for k, v in o.items()}

    res = {}
    for name, (p0, p1, flags) in batches.items():
        med, runs, o = dev_case(m, p0, p1, flags)
        vox = int(o["n_steps"].astype(np.int64).sum() + (o["status"] == 1).sum())  # (a stopped ray tested n_steps + 1 voxels)
        res[name] = o
        out["batches"][name] = {"flags": flags, "rays_ms": med, "rays_ms_runs": runs, "rays_per_s": N_RAYS / med * 1e3, "voxels_visited": vox,
                                "voxels_per_s": vox / med * 1e3, "stopped": int((o["status"] == 1).sum()), "n_unknown_sum": int(o["n_unknown"].sum())}
    # single-ray calls through the host mirror
    p0, p1, flags = batches["edges"]
    m.cast_rays(p0[:1], p1[:1], infl=True)
    t0 = time.perf_counter()
    K = 2000
    L, h = m._L, m._h
    st = np.zeros(1, np.int8)
    tt = np.zeros(1, np.float64)
    import ctypes
    for i in range(K):
        L.mlm_query_rays(h, ctypes.c_void_p(p0[i:i + 1].ctypes.data), ctypes.c_void_p(p1[i:i + 1].ctypes.data), 1, flags, ctypes.c_void_p(st.ctypes.data), None,
                         ctypes.c_void_p(tt.ctypes.data), None, None)
    out["mirror_us_per_ray"] = (time.perf_counter() - t0) / K * 1e6
    out["mirror_mean_voxels_per_ray"] = float((res["edges"]["n_steps"][:K] + (res["edges"]["status"][:K] == 1)).mean())
    out["host_queries"] = m.frame_stats()["n_host_queries"]
    m.close()
    # the yardstick, on a handle created with its knob
    mlmap.debug_set("mirror", 0)
    m3 = build_map()
    for name, (p0, p1, flags) in batches.items():
        Y = a.yard_rays
        ns = res[name]["n_steps"][:Y] + (res[name]["status"][:Y] == 1)
        ctr = np.ascontiguousarray(visited_centres(p0[:Y], p1[:Y], ns, cfg))
        assert len(ctr) == int(ns.sum())

        def yard():
            for i0 in range(0, len(ctr), 1 << 24):
                m3.getOccupancy(ctr[i0:i0 + (1 << 24)])
                m3.getInflateOccupancy(ctr[i0:i0 + (1 << 24)])

        med, runs = median3(yard, sync)
        c = out["batches"][name]
        c["yardstick_rays"] = Y
        c["yardstick_voxels"] = int(len(ctr))
        c["yardstick_ms"] = med
        c["yardstick_ms_runs"] = runs
        c["yardstick_voxels_per_s"] = len(ctr) / med * 1e3
        c["ratio_voxels_per_s"] = c["voxels_per_s"] / c["yardstick_voxels_per_s"]
    m3.close()
    mlmap.debug_reset()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
