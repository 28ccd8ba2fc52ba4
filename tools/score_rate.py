"""Rate of mlm_score_poses, beside what a client does today without it.

The map: the synthetic corridor (2 m wide, 3 m tall), S1, one frame per metre over 64 frames along a heading of --yaw degrees.  The
points: the corridor's VGA frame back-projected at step 8 (4 800 points) and at step 2 (76 800).  The poses, around the pose of frame
32: a correlative grid of 13 x 13 x 13 translations x 9 yaws (19 773 poses, pose_grid) and 256 random poses within +-0.5 m and +-10
degrees (a particle filter).  The field: mlm_export_esdf {sqdist}, OCC, max_dist 8, over the box of the points under the centre pose
grown by 12 voxels.  Device in, device out; the library runs on torch's stream so that device events bracket its work.  Per row,
median of --calls calls, host clock around call + synchronise (ms) and device events around the same call (dev_ms):
  - classes_ms, field_ms, both_ms: the call's three modes; pairs_per_s from both_ms;
  - today_classes_ms: (a) the n_poses x n_pts world positions by a torch expression on the device, copied to the host in chunks of
    2^24 positions, mlm_query_occupancy on each chunk, and a per-pose bincount of the answers — what the parent commit offers for the
    class counts; timed --cmp-calls times, and only while the row has at most 2^27 pairs;
  - today_field_ms: (b) with the same field already on the device: the torch transform in the contract's order in FP64, floor, box
    test, gather, clamp and per-pose sum, in chunks of poses that fit 2^27 pairs;
  - both comparators are checked equal to the call's table before they are timed (equal_classes, equal_field);
  - ratio_classes, ratio_field: today / call (> 1: mlm_score_poses is faster);
  - esdf_ms: mlm_export_esdf for the box, the other half of match_pose.
Prints one JSON document.
Usage: python tools/score_rate.py [--yaw 30] [--calls 30] [--cmp-calls 3] [--out profiles/score_rate.json]"""
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
from mlmapping_amd.mlmap import MLMap, backproject, compose_T_ws, pose_grid  # noqa: E402

FRAMES = 64
CMP_PAIRS = 1 << 27
OCC_CHUNK = 1 << 24


def build_map(yaw):
    m = MLMap(S1, max_blocks=65536, max_batch=8)
    img = syn.corridor_depth(S1)
    q = syn.quat_from_rpy(0.0, 0.0, yaw)
    for k in range(FRAMES):
        m.update_map(img, q, np.array([k * math.cos(yaw), k * math.sin(yaw), 1.5]))
    m.sync()
    return m, img, q


def timed(fn, calls):
    import torch

    fn()
    torch.cuda.synchronize()
    host, dev = [], []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return float(np.median(host)), float(np.median(dev))


def world(T, pts):
    """[k, j, 3] in the contract's operation order (elementwise torch operations: nothing fused)"""
    import torch

    out = []
    for a in range(3):
        t = T[:, 3 * a, None] * pts[None, :, 0]
        t = t + T[:, 3 * a + 1, None] * pts[None, :, 1]
        t = t + T[:, 3 * a + 2, None] * pts[None, :, 2]
        out.append(t + T[:, 9 + a, None])
    return torch.stack(out, dim=-1)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--yaw", type=float, default=30.0)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cmp-calls", type=int, default=3)
    ap.add_argument("--git", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    yaw = math.radians(a.yaw)
    d = S1.subbox_d_xyz
    m, img, q = build_map(yaw)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    L, h = m._L, m._h
    td = torch.tensor(d, dtype=torch.float64, device="cuda")
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "scene": "corridor", "frames": FRAMES, "yaw_deg": a.yaw, "blocks": m.block_count()}, "git": a.git or git or "unknown",
           "calls": a.calls, "cmp_calls": a.cmp_calls, "max_dist": 8, "sq_cap": 64, "rows": [],
           "not_measured": ["a wave-per-pose variant of k_score", "LDS point tiles other than 128", "a field larger than the L2 cache"]}
    T0 = compose_T_ws(q[None], np.array([[32 * math.cos(yaw), 32 * math.sin(yaw), 1.5]]), S1.T_B_S)[0]
    rng = np.random.default_rng(0)
    part = pose_grid(T0, d, (0, 0, 0), rng.uniform(-10, 10, size=256))
    part[:, 9:] += rng.uniform(-0.5, 0.5, size=(256, 3))
    pose_sets = {"grid 13x13x13 x 9 yaws": pose_grid(T0, d, (6, 6, 6), (-4, -3, -2, -1, 0, 1, 2, 3, 4)), "256 particles": part}
    K = (S1.cam_fx, S1.cam_fy, S1.cam_cx, S1.cam_cy)
    for step in (8, 2):
        pts = backproject(img, K, step)
        tp = torch.from_numpy(pts).cuda()
        w0 = np.floor((pts @ T0[:9].reshape(3, 3).T + T0[9:]) / d).astype(np.int64)
        lo, dims = w0.min(0) - 12, w0.max(0) - w0.min(0) + 25
        field = torch.empty(int(dims.prod()), dtype=torch.int32, device="cuda")
        esdf = timed(lambda: m.export_esdf_dev(lo, dims, 8, sqdist=field.data_ptr()), a.calls)
        tlo, tdims = torch.from_numpy(lo).cuda(), torch.from_numpy(dims).cuda()
        for name, T in pose_sets.items():
            tT = torch.from_numpy(np.ascontiguousarray(T)).cuda()
            n_poses, n_pts = len(T), len(pts)
            pairs = n_poses * n_pts
            table = torch.empty((n_poses, 8), dtype=torch.int64, device="cuda")
            run = lambda cl, fld: m.score_poses_dev(tp.data_ptr(), n_pts, tT.data_ptr(), n_poses, table.data_ptr(), cl, lo if fld else None,
                                                    dims if fld else None, field.data_ptr() if fld else None, 64)
            t_cls, t_fld, t_both = timed(lambda: run(True, False), a.calls), timed(lambda: run(False, True), a.calls), timed(lambda: run(True, True), a.calls)
            ref = table.cpu().numpy().copy()
            row = {"poses": name, "n_poses": n_poses, "n_pts": n_pts, "step": step, "pairs": pairs, "box_dims": [int(v) for v in dims],
                   "field_bytes": int(dims.prod()) * 4, "classes_ms": t_cls[0], "classes_dev_ms": t_cls[1], "field_ms": t_fld[0], "field_dev_ms": t_fld[1],
                   "both_ms": t_both[0], "both_dev_ms": t_both[1], "pairs_per_s": pairs / t_both[0] * 1e3, "esdf_ms": esdf[0], "esdf_dev_ms": esdf[1],
                   "match_pose_ms": esdf[0] + t_fld[0], "table_sums": ref.sum(0).tolist()}
            pose_chunk = max(1, CMP_PAIRS // n_pts)

            def today_field():
                cost = torch.empty(n_poses, dtype=torch.int64, device="cuda")
                for k0 in range(0, n_poses, pose_chunk):
                    # (a tensor divisor: torch divides by a Python scalar by multiplying with its reciprocal, which is not the contract's division)
                    v = (torch.floor(world(tT[k0:k0 + pose_chunk], tp) / td * 1024.0).to(torch.int64) >> 10) - tlo
                    inside = ((v >= 0) & (v < tdims)).all(dim=-1)
                    at = torch.where(inside, (v[..., 2] * tdims[1] + v[..., 1]) * tdims[0] + v[..., 0], 0)
                    c = torch.where(inside, field[at].clamp(0, 64).to(torch.int64), 64)
                    cost[k0:k0 + pose_chunk] = c.sum(dim=1)
                return cost

            row["equal_field"] = bool(torch.equal(today_field(), table[:, 6]))
            tf = timed(today_field, max(1, a.cmp_calls))
            row.update({"today_field_ms": tf[0], "ratio_field": tf[0] / t_fld[0]})
            if pairs <= CMP_PAIRS:
                occ_pose = max(1, OCC_CHUNK // n_pts)

                def today_classes():
                    counts = np.zeros((n_poses, 3), dtype=np.int64)
                    for k0 in range(0, n_poses, occ_pose):
                        pos = world(tT[k0:k0 + occ_pose], tp).reshape(-1, 3).cpu().numpy()
                        o = np.empty(len(pos), dtype=np.int8)
                        rc = L.mlm_query_occupancy(h, pos.ctypes.data_as(ctypes.c_void_p), len(pos), o.ctypes.data_as(ctypes.c_void_p))
                        assert rc == 0
                        k = np.repeat(np.arange(len(pos) // n_pts), n_pts)
                        counts[k0:k0 + occ_pose] = np.bincount(k * 3 + (o.astype(np.int64) + 1), minlength=3 * (len(pos) // n_pts)).reshape(-1, 3)
                    return counts  # columns: UNKNOWN, OCCUPIED, FREE

                run(True, False)
                torch.cuda.synchronize()
                cls = table.cpu().numpy()
                row["equal_classes"] = bool(np.array_equal(today_classes(), cls[:, [3, 1, 2]]))
                tc = timed(today_classes, max(1, a.cmp_calls))
                row.update({"today_classes_ms": tc[0], "ratio_classes": tc[0] / t_cls[0]})
            else:
                row["today_classes_ms"] = None  # (not measured: more than 2^27 pairs)
            row["wins"] = {"classes": None if row.get("ratio_classes") is None else ("mlm_score_poses" if row["ratio_classes"] > 1 else "mlm_query_occupancy + bincount"),
                           "field": "mlm_score_poses" if row["ratio_field"] > 1 else "torch gather"}
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
