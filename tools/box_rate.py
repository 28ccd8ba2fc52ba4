"""Rate of mlm_query_boxes, beside the only alternative a client has without it: point queries at the voxel centres of the boxes
(mlm_query_occupancy; plus mlm_query_inflate_occupancy when INFL is set — it is not, here).

The map: S1 after 48 room_jitter frames (inflate_map six times).  Two workloads, device in / device out:
  - grow:   4 096 single-voxel seeds in free space, max_grow 20 on all faces, OCC | UNKNOWN (a corridor planner's free boxes);
  - counts: 2^20 boxes of 4 x 4 x 4 voxels in the map's bounding box, max_grow NULL, OCC | UNKNOWN (pure counts).
Per workload, median of three runs each (same process, same map), host clock around call + synchronise:
  - boxes_ms: mlm_query_boxes (all four outputs), boxes/s and voxels of the final boxes/s (table word [0]);
  - yardstick_ms: the centres of the voxels of the FINAL boxes (enumerated on the host beforehand, not timed: the comparator is
    told the answer for free, so it bounds any query-based client from below) through one mlm_query_occupancy call per 2^24 centres,
    knob "mirror" = 0 — the upload of the centres is part of it: that is what the client pays.  Enumerating every voxel takes host
    memory (24 bytes each), so the yardstick runs on the first --yard-boxes boxes of the workload and is scaled by voxels;
  - ratio: yardstick time per voxel / mlm_query_boxes time per voxel of the final boxes (> 1: mlm_query_boxes is faster).
  - mirror_us_per_box: single-box calls of the grow workload with max_grow 4 through the host mirror (default knobs).
Prints one JSON document.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel's own times.
Usage: python tools/box_rate.py [--yard-boxes 256] [--out profiles/box_rate.json]"""
import argparse
import ctypes
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

N_SEEDS = 4096
N_COUNTS = 1 << 20
OCC, UNKNOWN = 1, 4


def build_map():
    m = MLMap(S1, max_blocks=16384, max_batch=8)
    frames = list(syn.stream(S1, "room_jitter", "smooth", 48))
    for k0 in range(0, 48, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
        m.inflate_map(fr[-1][1][1])
    m.sync()
    return m


def centres(boxes, cfg):
    """centres of all voxels of the inclusive boxes [K,6] (centre of v per axis: g * d_glb + c * d_sub + d_sub / 2)"""
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    out = []
    for b in boxes:
        ax = [np.arange(int(b[a]), int(b[3 + a]) + 1, dtype=np.int64) for a in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        out.append(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))
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
    ap.add_argument("--yard-boxes", type=int, default=256, help="boxes of the grow workload the yardstick runs on (64 times as many of counts)")
    ap.add_argument("--vgprs", type=int, default=-1, help="VGPR count of k_boxes from the build's resource usage remark")
    ap.add_argument("--git", default="", help="the commit the measured tree stands on (where the tool runs outside a checkout)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = S1
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    m = build_map()
    b = m.export_blocks()
    vlo, vhi = b["keys"].min(0) * n, (b["keys"].max(0) + 1) * n
    rng = np.random.default_rng(0)
    cand = rng.integers(vlo, vhi, size=(400000, 3))
    gq = np.floor_divide(cand, n)
    ctr = gq.astype(np.float64) * (d * n) + (cand - gq * n).astype(np.float64) * d + d * 0.5
    seeds = cand[m.getOccupancy(ctr) == 1][:N_SEEDS]
    assert len(seeds) == N_SEEDS, len(seeds)
    c0 = rng.integers(vlo, vhi - 3, size=(N_COUNTS, 3))
    work = {"grow": (np.concatenate([seeds, seeds], axis=1).astype(np.int32), 20, a.yard_boxes),
            "counts": (np.concatenate([c0, c0 + 3], axis=1).astype(np.int32), None, a.yard_boxes * 64)}
    sync = torch.cuda.synchronize
    git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"map": {"config": "S1", "frames": 48, "blocks": int(b["keys"].shape[0])}, "git": a.git or git or "unknown", "k_boxes_vgprs": a.vgprs,
           "flags": OCC | UNKNOWN, "workloads": {}}
    res = {}
    for name, (boxes, mg, _) in work.items():
        k = len(boxes)
        t_in = torch.from_numpy(boxes).cuda()
        o = {"status": torch.empty(k, dtype=torch.int8, device="cuda"), "box": torch.empty((k, 6), dtype=torch.int32, device="cuda"),
             "closed": torch.empty(k, dtype=torch.uint8, device="cuda"), "table": torch.empty((k, 4), dtype=torch.int64, device="cuda")}
        ptr = {key: v.data_ptr() for key, v in o.items()}
        med, runs = median3(lambda: m.query_boxes_dev(t_in.data_ptr(), k, occ=True, unknown=True, max_grow=mg, **ptr), sync)
        r = {key: v.cpu().numpy() for key, v in o.items()}
        res[name] = r
        vox = int(r["table"][:, 0].sum())
        out["workloads"][name] = {"boxes": k, "max_grow": mg, "boxes_ms": med, "boxes_ms_runs": runs, "boxes_per_s": k / med * 1e3, "final_voxels": vox,
                                  "voxels_per_s": vox / med * 1e3, "grown": int((r["status"] == 1).sum()), "blocked": int((r["status"] == 0).sum()),
                                  "slabs_absorbed": int(r["table"][:, 3].sum()), "unknown_voxels": int(r["table"][:, 1].sum())}
    # single-box calls through the host mirror
    boxes = work["grow"][0]
    mg4 = np.full(6, 4, np.int32)
    m.query_boxes(boxes[:1], unknown=True, max_grow=4)
    K = 2000
    L, h = m._L, m._h
    st, o6 = np.zeros(1, np.int8), np.zeros(6, np.int32)
    t0 = time.perf_counter()
    for i in range(K):
        L.mlm_query_boxes(h, ctypes.c_void_p(boxes[i:i + 1].ctypes.data), 1, OCC | UNKNOWN, ctypes.c_void_p(mg4.ctypes.data), None, None,
                          ctypes.c_void_p(st.ctypes.data), ctypes.c_void_p(o6.ctypes.data), None, None)
    out["mirror_us_per_box"] = (time.perf_counter() - t0) / K * 1e6
    out["host_queries"] = m.frame_stats()["n_host_queries"]
    m.close()
    # the yardstick, on a handle created with its knob
    mlmap.debug_set("mirror", 0)
    m3 = build_map()
    for name, (boxes, mg, Y) in work.items():
        fin = res[name]["box"][:Y]
        ctr = np.ascontiguousarray(centres(fin, cfg))
        assert len(ctr) == int(res[name]["table"][:Y, 0].sum())

        def yard():
            for i0 in range(0, len(ctr), 1 << 24):
                m3.getOccupancy(ctr[i0:i0 + (1 << 24)])

        med, runs = median3(yard, sync)
        c = out["workloads"][name]
        c["yardstick_boxes"] = int(Y)
        c["yardstick_voxels"] = int(len(ctr))
        c["yardstick_ms"] = med
        c["yardstick_ms_runs"] = runs
        c["yardstick_voxels_per_s"] = len(ctr) / med * 1e3
        c["yardstick_ms_scaled"] = med * c["final_voxels"] / len(ctr)
        c["ratio"] = c["yardstick_ms_scaled"] / c["boxes_ms"]
    m3.close()
    mlmap.debug_reset()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
