"""Rate of mlm_render_depth, beside the only alternative a client has without it: the segments of the same pixels materialised
(48 bytes per pixel of p0 / p1) and cast by mlm_query_rays.

The map: S1 after 48 room_jitter frames (inflate_map six times), as tools/ray_rate.py builds it.  Two workloads, MLM_RAY_OCC,
device in / device out:
  - fans:   4 096 poses x 64 x 48 (90 x 70 degrees) at 4 m — the candidate views of tools/view_rate.py: origins in free space, any
            yaw, pitch within +-0.5 rad;
  - frames: 64 poses x 640 x 480 with the configuration's camera at 8 m — the same kind of poses.
Per workload and per tile shape of k_render (knob "render_tile": 0 64 x 1, 1 16 x 4, 2 8 x 8; a handle and a map of its own each):
after two warm-up calls the median of --runs calls (host clock around call + synchronise), outputs depth + status only.  Beside
it, in the same process and on the same handle: mlm_query_rays over the segments of the same pixels (made here in numpy as the
contract states them, uploaded beforehand, not timed) with outputs status + t only, and the bytes of p0 / p1 it needed.  The two
are also held against each other (status equal, depth = the contract's formula on t), so the times are times of the same answers.
The runs of one workload alternate between the two calls.  Clocks: nothing is pinned; the warm-up calls and the alternation are
what keeps the comparison fair, and the spread of the runs is recorded.
Prints one JSON document.  Usage: python tools/render_rate.py [--runs 7] [--out profiles/render_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd import mlmap  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from tools.ray_rate import build_map  # noqa: E402
from tools.view_rate import rotations  # noqa: E402

TILES = {0: "64x1", 1: "16x4", 2: "8x8"}


def segments(T, width, height, K, mm):
    """p0, p1 (n * height * width, 3) as include/mlmap_hip.h states them (numpy fuses nothing)"""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    Z = np.float64(mm) / np.float64(1000.0)
    xs = ((np.arange(width, dtype=np.float64) - cx) * Z) / fx
    ys = ((np.arange(height, dtype=np.float64) - cy) * Z) / fy
    R, o = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
    p1 = np.empty((len(T), height, width, 3), dtype=np.float64)
    for a in range(3):
        r0, r1, r2, oa = (x[:, None, None] for x in (R[:, a, 0], R[:, a, 1], R[:, a, 2], o[:, a]))
        p1[..., a] = ((r0 * xs[None, None, :] + r1 * ys[None, :, None]) + r2 * Z) + oa
    p0 = np.ascontiguousarray(np.broadcast_to(o[:, None, None, :], p1.shape))
    return p0.reshape(-1, 3), p1.reshape(-1, 3)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--git", default="", help="the commit the measured tree stands on (where the tool runs outside a checkout)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = S1
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    sync = torch.cuda.synchronize
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "frames": 48}, "flags": 1, "runs": a.runs, "git": a.git or git or "unknown", "default_tile": None, "workloads": {}}
    work = None
    for tile, tname in TILES.items():
        mlmap.debug_set("render_tile", tile)
        m = build_map()
        mlmap.debug_reset()
        if work is None:  # the poses, once (the maps of the three handles are the same map)
            b = m.export_blocks()
            out["map"]["blocks"] = int(b["keys"].shape[0])
            lo, hi = b["keys"].min(0) * d * n, (b["keys"].max(0) + 1) * d * n
            rng = np.random.default_rng(0)
            cand = rng.uniform(lo, hi, size=(200000, 3))
            org = cand[m.getOccupancy(cand) == 1][:4096]
            assert len(org) == 4096, len(org)
            T = np.concatenate([rotations(rng, 4096).reshape(-1, 9), org], axis=1)
            work = {"fans": (T, 64, 48, (32.0 / np.tan(np.deg2rad(45.0)), 24.0 / np.tan(np.deg2rad(35.0)), 32.0, 24.0), 4000),
                    "frames": (np.ascontiguousarray(T[:64]), cfg.width, cfg.height, (cfg.cam_fx, cfg.cam_fy, cfg.cam_cx, cfg.cam_cy), 8000)}
        for name, (T, w, h, K, mm) in work.items():
            npx = len(T) * w * h
            c = out["workloads"].setdefault(name, {"poses": len(T), "width": w, "height": h, "max_depth_mm": mm, "pixels": npx, "pose_bytes": int(T.nbytes),
                                                   "segment_bytes": 48 * npx, "render_ms": {}, "render_ms_runs": {}, "rays_ms": {}, "rays_ms_runs": {}})
            dT = torch.from_numpy(T).cuda()
            depth = torch.zeros(npx, dtype=torch.int16, device="cuda")
            status = torch.zeros(npx, dtype=torch.int8, device="cuda")
            p0, p1 = segments(T, w, h, K, mm)
            d0, d1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
            del p0, p1
            r_status = torch.zeros(npx, dtype=torch.int8, device="cuda")
            r_t = torch.zeros(npx, dtype=torch.float64, device="cuda")
            render = lambda: m.render_depth_dev(dT.data_ptr(), len(T), w, h, K=K, max_depth=mm / 1000.0, depth=depth.data_ptr(), status=status.data_ptr())
            rays = lambda: m.cast_rays_dev(d0.data_ptr(), d1.data_ptr(), npx, status=r_status.data_ptr(), t=r_t.data_ptr())
            for _ in range(2):
                render(), sync(), rays(), sync()
            ts = {"render": [], "rays": []}
            for _ in range(a.runs):
                for key, fn in (("render", render), ("rays", rays)):
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    ts[key].append((time.perf_counter() - t0) * 1e3)
            # the same answers
            st, tt = r_status.cpu().numpy(), r_t.cpu().numpy()
            want = np.where(st == 1, np.clip(np.floor(tt * np.float64(mm) + 0.5), 1.0, 65535.0), 0.0).astype(np.uint16)
            assert np.array_equal(status.cpu().numpy(), st) and np.array_equal(depth.cpu().numpy().view(np.uint16), want), (name, tname)
            c["stopped"] = int((st == 1).sum())
            c["render_ms"][tname], c["render_ms_runs"][tname] = float(np.median(ts["render"])), [float(x) for x in ts["render"]]
            c["rays_ms"][tname], c["rays_ms_runs"][tname] = float(np.median(ts["rays"])), [float(x) for x in ts["rays"]]
            del dT, depth, status, d0, d1, r_status, r_t
            torch.cuda.empty_cache()
        m.close()
    for name, c in out["workloads"].items():
        best = min(c["render_ms"], key=c["render_ms"].get)
        c["fastest_tile"] = best
        c["rays_ms_median_of_handles"] = float(np.median(list(c["rays_ms"].values())))
        c["render_over_rays"] = {t: c["render_ms"][t] / c["rays_ms"][t] for t in c["render_ms"]}
        c["pixels_per_s"] = {t: c["pixels"] / c["render_ms"][t] * 1e3 for t in c["render_ms"]}
    import re
    k = int(re.search(r"kRenderTileDefault = (\d)", open(os.path.join(ROOT, "mlmapping_amd", "csrc", "mlm_handle.h")).read()).group(1))
    out["default_tile"] = TILES[k]  # (what a handle uses without the knob)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
