"""Rate of mlm_query_views, beside mlm_query_rays over the very same segments with only n_unknown requested (what a client summed
before; its sum over a fan is not the gain, see include/mlmap_hip.h).

The map is tools/ray_rate.py's: S1 after 48 room_jitter frames (inflate_map twice).  Device in, device out, MLM_RAY_OCC.
  a: 4 096 views of a 64 x 48 pinhole fan (90 x 70 degrees, 4 m) from origins in free space, any yaw, pitch within +-0.5 rad;
  b: ray_rate's "views" batch grouped per origin: 4 096 views of 256 random directions, 8 m;
  c: case a with a box around the map, an exclude array (30 % set) and mark.
Per case: two warm-up calls, then --runs timed calls each (host clock around call + synchronise; both calls return when their outputs
are written), reported as min / median / max; the table's sums; the overlap factor [6] / ([0] + [3]); an ESTIMATE of the views per bitset class
(recomputed here from floor(p / d) of the end points with the plan's thresholds, 8, 16, 32, 48, 64 KiB in LDS, larger in global
scratch: mlm_views.h decides, not this tool; the kernel trace shows the real launches, one k_views_lds per occupied class with that
class's LDS bytes and a workgroup per view).
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times; the difference between a
call's time and the sum of its kernels is the host side of the call (two stream synchronisations per chunk of 65 536 views: the
boxes come back for the plan).
Usage: python tools/view_rate.py [--views 4096] [--runs 7] [--out profiles/view_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import fan_views, pinhole_fan  # noqa: E402
from tools.ray_rate import build_map  # noqa: E402

CLASS_BYTES = (8192, 16384, 32768, 49152, 65472)


def timed(fn, sync, runs):
    for _ in range(2):
        fn()
        sync()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": float(np.min(ts)), "median_ms": float(np.median(ts)), "max_ms": float(np.max(ts)), "runs_ms": [float(t) for t in ts]}


def rotations(rng, count):
    yaw, pitch = rng.uniform(-np.pi, np.pi, count), rng.uniform(-0.5, 0.5, count)
    fwd = np.stack([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)], axis=1)
    right = np.stack([np.sin(yaw), -np.cos(yaw), np.zeros(count)], axis=1)
    return np.stack([right, np.cross(fwd, right), fwd], axis=2)


def classes(p0, p1, vb, d, box=None):
    """an estimate of the views per bitset class, from the boxes of the views' start and end voxels (cut to the box)"""
    v0, v1 = np.floor(p0 / d).astype(np.int64), np.floor(p1 / d).astype(np.int64)
    lo = np.minimum(np.minimum.reduceat(v0, vb[:-1]), np.minimum.reduceat(v1, vb[:-1]))
    hi = np.maximum(np.maximum.reduceat(v0, vb[:-1]), np.maximum.reduceat(v1, vb[:-1]))
    if box is not None:
        lo, hi = np.maximum(lo, np.array(box[0])), np.minimum(hi, np.array(box[0]) + np.array(box[1]) - 1)
    bits = np.prod(np.maximum(hi - lo + 1, 0), axis=1)
    nbytes = (bits + 31) // 32 * 4
    cls = np.searchsorted(np.array(CLASS_BYTES), nbytes)
    return {"lds_8k_16k_32k_48k_64k": [int((cls == c).sum()) for c in range(5)], "global": int((cls == 5).sum()),
            "bitset_kib_min_median_max": [float(nbytes.min() / 1024), float(np.median(nbytes) / 1024), float(nbytes.max() / 1024)]}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--git", default="", help="the commit the measured tree stands on (where the tool runs outside a checkout)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = S1
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    m = build_map()
    b = m.export_blocks()
    lo, hi = b["keys"].min(0) * d * n, (b["keys"].max(0) + 1) * d * n
    rng = np.random.default_rng(0)
    cand = rng.uniform(lo, hi, size=(200000, 3))
    org = cand[m.getOccupancy(cand) == 1][:a.views]
    assert len(org) == a.views, len(org)
    fan = pinhole_fan(64, 48, 32.0 / np.tan(np.deg2rad(45.0)), 24.0 / np.tan(np.deg2rad(35.0)), 32.0, 24.0, 4.0)
    u = rng.normal(size=(a.views, 256, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    box = ([int(x) for x in b["keys"].min(0) * n - 10], [int(x) for x in (b["keys"].max(0) - b["keys"].min(0) + 1) * n + 20])
    shape = box[1][::-1]
    cases = {"a": fan_views(org, rotations(rng, a.views), fan) + (None,),
             "b": (np.repeat(org, 256, axis=0), (org[:, None, :] + 8.0 * u).reshape(-1, 3), (np.arange(a.views + 1) * 256).astype(np.int32), None)}
    cases["c"] = cases["a"][:3] + (box,)
    sync = torch.cuda.synchronize
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "frames": 48, "blocks": int(b["keys"].shape[0])}, "views": a.views, "flags": 1, "git": a.git or git or "unknown",
           "cases": {}}
    for name, (p0, p1, vb, bx) in cases.items():
        nr = len(p0)
        t0, t1, tvb = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), torch.from_numpy(vb).cuda()
        table = torch.zeros((a.views, 8), dtype=torch.int64, device="cuda")
        kw = {}
        if bx is not None:
            ex = torch.from_numpy((rng.random(shape) < 0.3).astype(np.uint8)).cuda()
            mark = torch.zeros(shape, dtype=torch.uint8, device="cuda")
            kw = {"box": bx, "exclude": ex.data_ptr(), "mark": mark.data_ptr()}
        views = timed(lambda: m.query_views_dev(t0.data_ptr(), t1.data_ptr(), tvb.data_ptr(), a.views, occ=True, table=table.data_ptr(), **kw), sync, a.runs)
        t = table.cpu().numpy()
        nu = torch.zeros(nr, dtype=torch.int32, device="cuda")
        rays = timed(lambda: m.cast_rays_dev(t0.data_ptr(), t1.data_ptr(), nr, occ=True, n_unknown=nu.data_ptr()), sync, a.runs)
        c = {"rays": nr, "rays_per_view": nr // a.views, "box": bx, "query_views": views, "query_rays_n_unknown": rays,
             "ratio_median": views["median_ms"] / rays["median_ms"], "views_per_s": a.views / views["median_ms"] * 1e3,
             "table_sums": [int(x) for x in t.sum(0)], "overlap_factor": float(t[:, 6].sum() / max(1, t[:, 0].sum() + t[:, 3].sum())),
             "sum_of_per_ray_n_unknown": int(nu.sum().item()), "classes_estimated_from_end_points": classes(p0, p1, vb, d, bx)}
        if bx is not None:
            c["marked_voxels"] = int((mark != 0).sum().item())
        out["cases"][name] = c
        del t0, t1, nu
    out["device_bytes"] = int(m.frame_stats()["device_bytes"])
    m.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
