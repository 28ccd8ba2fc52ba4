"""Rate of mlm_export_octree beside what a caller does without it: export_window_dev {occ} of the same box and the label pyramid built
from it in torch.

The map: 64 frames of the S1 corridor stream.  The box: 512 x 512 x 64 voxels round the vehicle, depth 16.  Flags 0 and OCC_ONLY.
Device in, device out.  Per flags, in ONE loop that alternates the calls, each timed with the host clock around call + synchronise
after warm-up calls of every shape:
  - octree_words_ms:  mlm_export_octree {words};
  - octree_all_ms:    mlm_export_octree {words, inner4, skip, leaf4, leaf_class};
  - octree_size_ms:   mlm_export_octree {summary} alone, the sizing call;
  - torch_pyramid_ms: export_window_dev {occ}, the labels of the voxels, then per level the array padded to even cell coordinates,
                      reshaped into 2 x 2 x 2 groups, amin / amax over a group and the parent's label from the two.  It numbers
                      nothing and writes no word and no leaf, so it is a lower bound of the detour.  Its count of inner cells is
                      checked equal to the call's N before anything is timed.
Reported: median, min and max of the calls, N and M, the ratio torch_pyramid / octree_all of the medians — whichever way it falls.
Writes one JSON document.  Usage: python tools/octree_rate.py [--reps 30] [--warmup 3] [--out profiles/octree_rate.json]"""
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

DIMS = (512, 512, 64)
DEPTH = 16
CASES = {"OCC+FREE": dict(), "OCC_ONLY": dict(occ_only=True)}


def torch_pyramid(torch, m, lo, dims, occ, occ_only):
    """the labels of every level from the occ classes of the box (occ: int8 device tensor [dz][dy][dx]); returns the inner cells"""
    import torch.nn.functional as F

    m.export_window_dev(lo, dims, occ=occ.data_ptr())
    lab = torch.where(occ == 0, 2, 0).to(torch.uint8) if occ_only else torch.where(occ == 0, 2, torch.where(occ == 1, 1, 0)).to(torch.uint8)
    org = [lo[a] + (1 << (DEPTH - 1)) for a in range(3)]
    inner = torch.zeros((), dtype=torch.int64, device=occ.device)
    for _ in range(DEPTH):
        before = [org[a] & 1 for a in range(3)]
        after = [(before[a] + lab.shape[2 - a]) & 1 for a in range(3)]
        lab = F.pad(lab, (before[0], after[0], before[1], after[1], before[2], after[2]))
        nz, ny, nx = (s // 2 for s in lab.shape)
        g = lab.reshape(nz, 2, ny, 2, nx, 2).permute(0, 2, 4, 1, 3, 5).reshape(nz, ny, nx, 8)
        low, high = g.amin(dim=3), g.amax(dim=3)
        lab = torch.where(high == 0, 0, torch.where((low == high) & (low != 3), low, 3)).to(torch.uint8)
        inner += (lab == 3).sum()
        org = [(org[a] - before[a]) >> 1 for a in range(3)]
    return inner


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "octree_rate.json"))
    a = ap.parse_args()
    cfg = S1
    m = MLMap(cfg, max_blocks=16384, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    vehicle = [int(np.floor(v / cfg.subbox_d_xyz)) for v in frames[-1][1][1]]
    dims = list(DIMS)
    lo = [int(vehicle[i] - dims[i] // 2) for i in range(3)]
    sync = torch.cuda.synchronize
    occ = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.int8, device="cuda")
    out = {"map": {"config": "S1", "scene": "corridor", "frames": 64, "blocks": m.block_count()}, "lo": lo, "dims": dims, "depth": DEPTH,
           "voxels": int(np.prod(dims)), "reps": a.reps, "warmup": a.warmup, "cases": {}}
    for name, flags in CASES.items():
        sm = m.export_octree_dev(lo, dims, DEPTH, **flags)
        N, M = int(sm[0]), int(sm[1])
        words = torch.empty(max(N, 1), dtype=torch.int16, device="cuda")
        inner4 = torch.empty((max(N, 1), 4), dtype=torch.int32, device="cuda")
        skip = torch.empty(max(N, 1), dtype=torch.int32, device="cuda")
        leaf4 = torch.empty((max(M, 1), 4), dtype=torch.int32, device="cuda")
        leaf_class = torch.empty(max(M, 1), dtype=torch.int8, device="cuda")
        fns = {
            "octree_words_ms": lambda: m.export_octree_dev(lo, dims, DEPTH, words=words.data_ptr(), cap_inner=max(N, 1), summary=False, **flags),
            "octree_all_ms": lambda: m.export_octree_dev(lo, dims, DEPTH, words=words.data_ptr(), inner4=inner4.data_ptr(), skip=skip.data_ptr(),
                                                         cap_inner=max(N, 1), leaf4=leaf4.data_ptr(), leaf_class=leaf_class.data_ptr(),
                                                         cap_leaves=max(M, 1), summary=False, **flags),
            "octree_size_ms": lambda: m.export_octree_dev(lo, dims, DEPTH, **flags),
            "torch_pyramid_ms": lambda: torch_pyramid(torch, m, lo, dims, occ, bool(flags.get("occ_only"))),
        }
        assert int(fns["torch_pyramid_ms"]()) == N, "the comparator's inner cells differ from the call's N"
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        sync()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():  # (alternating: the calls see the same machine)
                t0 = time.perf_counter()
                fn()
                sync()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        row = {k: stats(v) for k, v in ts.items()}
        row.update(N=N, M=M, summary=[int(v) for v in sm], ratio_torch_over_octree_all=row["torch_pyramid_ms"]["median"] / row["octree_all_ms"]["median"])
        out["cases"][name] = row
    m.close()
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
