"""Rate of mlm_export_mesh beside what a caller does without it: export_window_dev {occ, infl} of the box grown by one voxel and the
face list built from it in torch.

The map: 64 frames of the S1 corridor stream.  The box: 512 x 512 x 64 voxels round the vehicle.  Flags OCC and OCC | SEEN.  Device
in, device out.  Per flags, in ONE loop that alternates the three, each timed with the host clock around call + synchronise after
warm-up calls of every shape:
  - mesh_faces_ms:  mlm_export_mesh {quads, face4};
  - mesh_all_ms:    mlm_export_mesh {quads, face4, vert3, vert_xyz, vert_n3};
  - torch_faces_ms: export_window_dev {occ, infl} of the grown box, then shifted comparisons of the class arrays, nonzero, and a sort
                    by the face key linear(v) * 6 + a: faces only, it numbers no vertices, so it is a lower bound of the detour.  Its
                    rows are checked equal to the call's face4 before anything is timed.
Reported: median, min and max of the calls, F and V, the ratio torch_faces / mesh_faces of the medians.
Writes one JSON document.  Usage: python tools/mesh_rate.py [--reps 30] [--warmup 3] [--out profiles/mesh_rate.json]"""
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
CASES = {"OCC": dict(occ=True), "OCC|SEEN": dict(occ=True, seen=True)}


def torch_faces(torch, m, lo, dims, occ, infl, seen):
    """face4 rows of the box from the classes of the grown box (occ, infl: int8 device tensors [dz + 2][dy + 2][dx + 2]), flags OCC
    [| SEEN]"""
    m.export_window_dev([v - 1 for v in lo], [v + 2 for v in dims], occ=occ.data_ptr(), infl=infl.data_ptr())
    obstacle = occ == 0
    is_open = (occ == 1) if seen else ~obstacle
    core = obstacle[1:-1, 1:-1, 1:-1]
    sl = [slice(0, -2), slice(1, -1), slice(2, None)]
    keys = []
    for a in range(6):
        d = [0, 0, 0]
        d[a >> 1] = 1 if a & 1 else -1
        lin = torch.nonzero((core & is_open[sl[d[2] + 1], sl[d[1] + 1], sl[d[0] + 1]]).reshape(-1)).reshape(-1)
        keys.append(lin * 6 + a)
    key = torch.sort(torch.cat(keys)).values
    lin, a = torch.div(key, 6, rounding_mode="floor"), key % 6
    x, y, z = lin % dims[0], torch.div(lin, dims[0], rounding_mode="floor") % dims[1], torch.div(lin, dims[0] * dims[1], rounding_mode="floor")
    return torch.stack([x + lo[0], y + lo[1], z + lo[2], a], dim=1).to(torch.int32)


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mesh_rate.json"))
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
    grown = (dims[2] + 2, dims[1] + 2, dims[0] + 2)
    occ = torch.empty(grown, dtype=torch.int8, device="cuda")
    infl = torch.empty(grown, dtype=torch.int8, device="cuda")
    out = {"map": {"config": "S1", "scene": "corridor", "frames": 64, "blocks": m.block_count()}, "lo": lo, "dims": dims, "voxels": int(np.prod(dims)),
           "reps": a.reps, "warmup": a.warmup, "cases": {}}
    for name, flags in CASES.items():
        sm = m.export_mesh_dev(lo, dims, **flags)
        F, V = int(sm[0]), int(sm[1])
        quads = torch.empty((F, 4), dtype=torch.int32, device="cuda")
        face4 = torch.empty((F, 4), dtype=torch.int32, device="cuda")
        vert3 = torch.empty((V, 3), dtype=torch.int32, device="cuda")
        xyz = torch.empty((V, 3), dtype=torch.float32, device="cuda")
        n3 = torch.empty((V, 3), dtype=torch.int8, device="cuda")
        fns = {
            "mesh_faces_ms": lambda: m.export_mesh_dev(lo, dims, quads=quads.data_ptr(), faces=face4.data_ptr(), cap_faces=F, summary=False, **flags),
            "mesh_all_ms": lambda: m.export_mesh_dev(lo, dims, quads=quads.data_ptr(), faces=face4.data_ptr(), cap_faces=F, verts=vert3.data_ptr(),
                                                     xyz=xyz.data_ptr(), normals=n3.data_ptr(), cap_verts=V, summary=False, **flags),
            "torch_faces_ms": lambda: torch_faces(torch, m, lo, dims, occ, infl, bool(flags.get("seen"))),
        }
        fns["mesh_faces_ms"]()
        sync()
        assert torch.equal(fns["torch_faces_ms"](), face4), "the comparator's face list differs from the call's face4"
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        sync()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():  # (alternating: the three see the same machine)
                t0 = time.perf_counter()
                fn()
                sync()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        row = {k: stats(v) for k, v in ts.items()}
        row.update(F=F, V=V, summary=[int(v) for v in sm], ratio_torch_over_mesh_faces=row["torch_faces_ms"]["median"] / row["mesh_faces_ms"]["median"])
        out["cases"][name] = row
    m.close()
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
