"""Rate of mlm_query_clearance — the distance field of a batch's box plus the walk through it — beside mlm_query_sweeps and mlm_query_rays.

The map, the edges, the radii, the batch sizes and the timing rule are tools/sweep_rate.py's: the synthetic corridor (2 m wide, 3 m tall),
S1, one frame per metre over 64 frames along a heading of --yaw degrees; both end points uniform in the map's bounding box, 2^16 and 2^20
edges, device in / device out, OCC, radius 0, 1, 2, 4, 8 and 16.  Per row, median of 30 calls after 2 warm-ups (same process, same
map, one loop), host clock around call + synchronise:
  - esdf_ms: mlm_export_esdf {sqdist} at max_dist r + 1 over the voxel bounding box of the batch, into device memory;
  - clear1_ms, clearK_ms: mlm_query_clearance on that field with sq_stop r^2, sq_cap (r + 1)^2, all eight outputs, with the knob
    clear_ahead 1 and K = 4 (two handles with the same map: the knob is read by mlm_create);
  - field_walk1_ms, field_walkK_ms: esdf_ms plus each of them — what an edge check through the field costs;
  - sweeps_ms: mlm_query_sweeps at radius r, all seven outputs; rays_ms: mlm_query_rays, OCC, all five outputs, on the same edges;
  - sweeps_over_field_walk: sweeps_ms over the better of the two sums (> 1: field plus walk is faster); walk_over_rays: the better walk
    over rays_ms (what a load per voxel costs beside a probe per block).
Before a row is timed, status, voxel3, t and n_steps of both walks are checked equal to mlm_query_sweeps' (every path lies in the box).
One grouped row: the first 2^16 edges as 4 096 groups of 16 consecutive segments, radius 2, the table alone.
Prints one JSON document.  Usage: python tools/clearance_rate.py [--yaw 30] [--calls 30] [--out profiles/clearance_rate.json]"""
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

from mlmapping_amd import mlmap as mm  # noqa: E402
from mlmapping_amd import synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402

COUNTS = (1 << 16, 1 << 20)
RADII = (0, 1, 2, 4, 8, 16)
FRAMES = 64
AHEAD = 4
WARMUPS = 2


def build_map(yaw, ahead):
    mm.debug_set("clear_ahead", ahead)
    m = MLMap(S1, max_blocks=65536, max_batch=8)
    img = syn.corridor_depth(S1)
    q = syn.quat_from_rpy(0.0, 0.0, yaw)
    for k in range(FRAMES):
        m.update_map(img, q, np.array([k * math.cos(yaw), k * math.sin(yaw), 1.5]))
    m.sync()
    return m


def median_of(fn, sync, calls):
    for _ in range(WARMUPS):
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
    maps = {1: build_map(yaw, 1), AHEAD: build_map(yaw, AHEAD)}
    m = maps[1]
    b = m.export_blocks()
    lo_w, hi_w = b["keys"].min(0) * d * n, (b["keys"].max(0) + 1) * d * n
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "scene": "corridor", "frames": FRAMES, "yaw_deg": a.yaw, "blocks": int(b["keys"].shape[0])}, "git": a.git or git or "unknown",
           "flags": 1, "calls": a.calls, "warmups": WARMUPS, "ahead": AHEAD, "rows": []}
    rng = np.random.default_rng(0)
    vp = ctypes.c_void_p
    P = lambda t: vp(t.data_ptr())
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    same = ("status", "voxel", "t", "n_steps")
    for count in COUNTS:
        p0, p1 = rng.uniform(lo_w, hi_w, size=(count, 3)), rng.uniform(lo_w, hi_w, size=(count, 3))
        t0, t1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
        sw = {"status": torch.empty(count, dtype=torch.int8, device="cuda"), "voxel": i32(count, 3), "t": torch.empty(count, dtype=torch.float64, device="cuda"),
              "n_steps": i32(count), "n_unknown": i32(count), "hit": i32(count, 3), "hit_sq": i32(count)}
        cl = {"status": torch.empty(count, dtype=torch.int8, device="cuda"), "voxel": i32(count, 3), "t": torch.empty(count, dtype=torch.float64, device="cuda"),
              "n_steps": i32(count), "min_sq": i32(count), "min": i32(count, 3), "cost": torch.empty(count, dtype=torch.int64, device="cuda"), "n_near": i32(count)}
        sw_ptr = [P(sw[k]) for k in ("status", "voxel", "t", "n_steps", "n_unknown", "hit", "hit_sq")]
        cl_ptr = [P(cl[k]) for k in ("status", "voxel", "t", "n_steps", "min_sq", "min", "cost", "n_near")]
        ray_ptr = {k: sw[k].data_ptr() for k in ("status", "voxel", "t", "n_steps", "n_unknown")}
        vox = np.floor(np.floor((np.concatenate([p0, p1]) / d) * 1024.0) / 1024.0).astype(np.int64)
        blo, dims = vox.min(0), vox.max(0) - vox.min(0) + 1
        box_voxels = int(dims.prod())
        lo_c, dims_c = np.ascontiguousarray(blo, dtype=np.int32), np.ascontiguousarray(dims, dtype=np.int32)
        field = torch.empty(box_voxels, dtype=torch.int32, device="cuda")
        L = m._L
        rays = median_of(lambda: m.cast_rays_dev(t0.data_ptr(), t1.data_ptr(), count, occ=True, **ray_ptr), sync, a.calls)

        def walk(k, r, outs=cl_ptr, gb=None, ng=0, table=None, cnt=count):
            rc = L.mlm_query_clearance(maps[k]._h, P(t0), P(t1), cnt, mm._p(lo_c), mm._p(dims_c), P(field), r * r, (r + 1) ** 2, 0, *outs, gb, ng, table)
            assert rc == 0, (rc, L.mlm_last_error(maps[k]._h))

        for r in RADII:
            assert L.mlm_query_sweeps(m._h, P(t0), P(t1), count, r, 1, *sw_ptr) == 0
            m.export_esdf_dev(blo, dims, r + 1, sqdist=field.data_ptr())
            sync()
            for k in (1, AHEAD):  # the walk's stop bytes are the sweep's
                for t in cl.values():
                    t.zero_()
                walk(k, r)
                sync()
                for name in same:
                    assert torch.equal(cl[name], sw[name]), f"clear_ahead {k}, radius {r}: {name} differs from mlm_query_sweeps"
            st = sw["status"].cpu().numpy()
            path_voxels = int(cl["n_steps"].to(torch.int64).sum())  # (voxels the walk passed)
            sweeps = median_of(lambda: L.mlm_query_sweeps(m._h, P(t0), P(t1), count, r, 1, *sw_ptr), sync, a.calls)
            esdf = median_of(lambda: m.export_esdf_dev(blo, dims, r + 1, sqdist=field.data_ptr()), sync, a.calls)
            c1 = median_of(lambda: walk(1, r), sync, a.calls)
            ck = median_of(lambda: walk(AHEAD, r), sync, a.calls)
            best = min(c1[0], ck[0])
            row = {"edges": count, "radius": r, "box_dims": [int(v) for v in dims], "box_voxels": box_voxels, "passed_voxels": path_voxels,
                   "stopped": int((st == 1).sum()), "not_stopped": int((st == 0).sum()), "esdf_ms": esdf[0], "esdf_ms_min_max": esdf[1:],
                   "clear1_ms": c1[0], "clear1_ms_min_max": c1[1:], "clearK_ms": ck[0], "clearK_ms_min_max": ck[1:],
                   "field_walk1_ms": esdf[0] + c1[0], "field_walkK_ms": esdf[0] + ck[0], "sweeps_ms": sweeps[0], "sweeps_ms_min_max": sweeps[1:],
                   "rays_ms": rays[0], "rays_ms_min_max": rays[1:], "sweeps_over_field_walk": sweeps[0] / (esdf[0] + best), "walk_over_rays": best / rays[0],
                   "K_over_1": ck[0] / c1[0]}
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        if count == COUNTS[0]:  # the grouped row: 4 096 groups of 16 consecutive segments, the table alone
            r, ng = 2, count // 16
            gb = torch.arange(0, count + 1, 16, dtype=torch.int32, device="cuda")
            table = torch.empty((ng, 8), dtype=torch.int64, device="cuda")
            m.export_esdf_dev(blo, dims, r + 1, sqdist=field.data_ptr())
            none = [None] * 8
            g1 = median_of(lambda: walk(1, r, none, P(gb), ng, P(table)), sync, a.calls)
            gk = median_of(lambda: walk(AHEAD, r, none, P(gb), ng, P(table)), sync, a.calls)
            tab = table.cpu().numpy()
            out["grouped"] = {"edges": count, "groups": ng, "segments_per_group": 16, "radius": r, "clear1_ms": g1[0], "clear1_ms_min_max": g1[1:],
                              "clearK_ms": gk[0], "clearK_ms_min_max": gk[1:], "groups_blocked": int((tab[:, 1] >= 0).sum())}
            print(json.dumps(out["grouped"]), file=sys.stderr, flush=True)
    for g in maps.values():
        g.close()
    # the expectation: field plus walk takes less time than mlm_query_sweeps at every radius >= 1 of the table
    losing = [(r["edges"], r["radius"]) for r in out["rows"] if r["radius"] >= 1 and r["sweeps_over_field_walk"] <= 1.0]
    out["faster_than_sweeps_at_every_radius_ge_1"] = not losing
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    if losing:
        sys.exit(f"field plus walk is not faster than mlm_query_sweeps at (edges, radius) {losing}")


if __name__ == "__main__":
    main()
