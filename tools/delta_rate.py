"""Rate of mlm_delta_blocks beside the two ways to find the changed blocks without it:
  (a) host:   export_blocks of the whole map to the host and a numpy row comparison with the kept previous dump;
  (b) device: mlm_export_blocks into torch device tensors and a torch row comparison with a kept previous device copy — the map held
              twice more on the device (the copy of now, the copy of before).
Both comparators compare slot by slot, which names the right blocks only while old blocks keep their slots — true of every change made
here (whole blocks overwritten in place, frames integrated: new blocks go behind), not after a crop, an aging that drops or a reanchor.

The maps: 64 frames of the S1 corridor stream, and the crafted map of 16 384 blocks tools/crop_rate.py .. age_rate.py use.  Between the
table and the timed calls 0 %, 1 %, 10 % or 100 % of the blocks, chosen at random, get one log-odds value changed (import_blocks of those
blocks), or — corridor map only — one more frame is integrated.  The timed calls do not change the map, so every repetition does the same
work.  Per map and change, in ONE loop that alternates the calls, each timed with the host clock around call + synchronise:
  - delta_dev_ms:   MLMap.delta with the previous table and every output in device memory (the dry call that sizes included);
  - delta_host_ms:  the same with the previous table and every output in host memory (staged);
  - delta_dry_ms:   the dry call alone: digests, sort, join, counts;
  - host_ms, device_ms: the comparators.
Before anything is timed each comparator must name the block set the call emits.  Every delta row reports the bytes by the rule's own
count — 6 read per voxel of a selected block and 12 per key, 6 written per voxel of an emitted block, 28 per table row — and the
bytes/s that makes of the median, beside the HBM peak.  Writes one JSON document.
Usage: python tools/delta_rate.py [--reps 30] [--warmup 2] [--cmp-reps 3] [--out profiles/delta_rate.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd import synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
KEY_MIN = -(1 << 20)
WHOLE = ([KEY_MIN] * 3, [1 << 21] * 3)
MAX_BLOCKS = 16384
PLANES = ("keys", "log_odds", "occ", "infl")


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "reps": len(ts)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cmp-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delta_rate.json"))
    a = ap.parse_args()
    cfg = S1
    C = cfg.cells_per_block
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    out = {"hbm_peak_GBs": HBM_PEAK_GBS, "reps": a.reps, "warmup": a.warmup, "maps": {}, "cases": {},
           "not_measured": ["a key box (an unselected block costs one key read and its entry of the sort)", "MLM_DELTA_NO_INFL (the same reads)",
                            "subbox_n other than 10 (the one-voxel lane path of subbox_n 2, 3, 5, 7, 9)", "gone keys, and a replica applying the delta",
                            "the crafted map with a frame integrated", "calls while frames are in flight (the call drains them first)",
                            "the kernels on their own (host clock around the whole call only)", "a radio link or a second GPU on the receiving end"]}

    def raw_export_dev(m, nb):
        t = {"keys": torch.empty((nb, 3), dtype=torch.int32, device="cuda"), "log_odds": torch.empty((nb, C), dtype=torch.float32, device="cuda"),
             "occ": torch.empty((nb, C), dtype=torch.uint8, device="cuda"), "infl": torch.empty((nb, C), dtype=torch.uint8, device="cuda")}
        n_out = ctypes.c_int32()
        m._chk(m._L.mlm_export_blocks(m._h, nb, *[ctypes.c_void_p(t[k].data_ptr()) for k in PLANES], ctypes.byref(n_out)), "mlm_export_blocks")
        return t

    def run_case(tag, m, mutate):
        """the table and both previous copies, the mutation, then the loop"""
        nb0 = m.block_count()
        t_dev = m.delta(device=True).table
        t_host = tuple(x.cpu().numpy() for x in t_dev)
        t_host = (t_host[0], t_host[1].view(np.uint64))
        prev_host = m.export_blocks(raw=True)
        prev_dev = raw_export_dev(m, nb0)
        sync()
        mutate()
        m.sync()
        nb = m.block_count()

        def host_way():
            t0 = time.perf_counter()
            now = m.export_blocks(raw=True)
            diff = (now["log_odds"][:nb0].view(np.uint32) != prev_host["log_odds"].view(np.uint32)).any(axis=1)
            diff |= (now["occ"][:nb0] != prev_host["occ"]).any(axis=1) | (now["infl"][:nb0] != prev_host["infl"]).any(axis=1)
            keys = np.concatenate([now["keys"][:nb0][diff], now["keys"][nb0:]])
            return (time.perf_counter() - t0) * 1e3, keys

        def device_way():
            sync()
            t0 = time.perf_counter()
            now = raw_export_dev(m, nb)
            diff = (now["log_odds"][:nb0].view(torch.int32) != prev_dev["log_odds"].view(torch.int32)).any(dim=1)
            diff |= (now["occ"][:nb0] != prev_dev["occ"]).any(dim=1) | (now["infl"][:nb0] != prev_dev["infl"]).any(dim=1)
            keys = torch.cat([now["keys"][:nb0][diff], now["keys"][nb0:]])
            sync()
            return (time.perf_counter() - t0) * 1e3, keys.cpu().numpy()

        def timed(fn):
            sync()
            t0 = time.perf_counter()
            r = fn()
            sync()
            return (time.perf_counter() - t0) * 1e3, r

        calls = {"delta_dev_ms": lambda: m.delta(prev=t_dev, device=True), "delta_host_ms": lambda: m.delta(prev=t_host),
                 "delta_dry_ms": lambda: m.delta(prev=t_dev, dry=True)}
        # the same block set on every side before anything is timed
        d = m.delta(prev=t_host)
        assert np.array_equal(m.export_blocks(raw=True)["keys"][:nb0], prev_host["keys"]), "old blocks left their slots"
        named = {tuple(k) for k in d.keys.tolist()}
        for way in (host_way, device_way):
            assert {tuple(k) for k in way()[1].tolist()} == named, f"{way.__name__} names another block set"
        sm = [int(v) for v in d.summary]
        ts = {k: [] for k in list(calls) + ["host_ms", "device_ms"]}
        for r in range(a.warmup + a.reps):
            for k, fn in calls.items():
                dt, _ = timed(fn)
                if r >= a.warmup:
                    ts[k].append(dt)
            dt, _ = device_way()
            if r >= a.warmup:
                ts["device_ms"].append(dt)
            if len(ts["host_ms"]) < a.cmp_reps:  # (in the same loop; up to seconds per call on the large map, so fewer of them and no warm-up)
                ts["host_ms"].append(host_way()[0])
        row = {k: stats(v) for k, v in ts.items() if v}
        S, E = sm[1], sm[5] + sm[6]
        for k in calls:
            med = row[k]["median"]
            b = S * (6 * C + 12) + (0 if k == "delta_dry_ms" else E * (6 * C + 13) + S * 28 + sm[2] * 28)
            row[k].update(rule_bytes=b, achieved_GBs=b / (med * 1e-3) / 1e9, fraction_of_hbm_peak=b / (med * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          host_over_call=row["host_ms"]["median"] / med, device_over_call=row["device_ms"]["median"] / med)
        row.update(blocks=nb, emitted_blocks=E, map_bytes=nb * (12 + 6 * C), emitted_bytes=E * (13 + 6 * C), table_bytes=S * 28, summary=sm)
        out["cases"][tag] = row
        print(tag, json.dumps({k: v["median"] for k, v in row.items() if isinstance(v, dict)}), flush=True)

    def run_map(tag, m, with_frame):
        base = m.export_blocks(raw=True)
        nb = len(base["keys"])
        out["maps"][tag].update(blocks=nb, cells=C, map_bytes=nb * (12 + 6 * C))
        for pct in (0, 1, 10, 100):
            pick = rng.permutation(nb)[:int(round(pct / 100 * nb))]

            def mutate(pick=pick):
                if len(pick):
                    lo = base["log_odds"][pick].copy()
                    lo[:, 0] = np.where(lo[:, 0] == np.float32(0.125), np.float32(0.25), np.float32(0.125))
                    m.import_blocks(base["keys"][pick], lo, base["occ"][pick], base["infl"][pick])
            run_case(f"{tag}_p{pct}", m, mutate)
            if len(pick):  # the map back as it was, so the next level changes its own share only
                m.import_blocks(base["keys"][pick], base["log_odds"][pick], base["occ"][pick], base["infl"][pick])
        if with_frame is not None:
            run_case(f"{tag}_frame", m, with_frame)

    out["maps"]["corridor"] = {"config": "S1", "scene": "corridor", "frames": 64}
    m = MLMap(cfg, max_blocks=MAX_BLOCKS, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 65))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    run_map("corridor", m, lambda: m.update_map(frames[64][0], *frames[64][1]))
    m.close()
    out["maps"]["crafted"] = {"config": "S1", "scene": "32 x 32 x 16 block keys, random planes"}
    big = MLMap(cfg, max_blocks=4 * MAX_BLOCKS, max_batch=8)
    kx, ky, kz = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing="ij")
    keys = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.int32)[rng.permutation(MAX_BLOCKS)]
    big.import_blocks(keys, rng.uniform(-2.0, 4.0, size=(MAX_BLOCKS, C)).astype(np.float32), rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(MAX_BLOCKS, C)),
                      rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(MAX_BLOCKS, C)))
    run_map("crafted", big, None)
    big.close()
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
