"""Size and rate of mlm_pack_blocks / mlm_unpack_blocks beside three ways to make a map small without them:
  (a) numpy:  export_blocks of the whole map to the host and the contract's numpy encoder (tests/pack_ref.py) — the same bytes;
  (b) zlib:   export_blocks to the host and zlib.compress(level=1) over the dump (keys, log-odds, occ, infl) — its size is reported too;
  (c) torch:  mlm_export_blocks into torch device tensors and a compaction of the log-odds alone (`!= 0` mask, nonzero, gather) — a
              lower bound that writes no stream and leaves occ and infl at a byte per voxel.
Each is first checked to round-trip the same blocks.

The maps: 64 frames of the S1 corridor stream, and the crafted map of 16 384 blocks of random planes tools/crop_rate.py .. delta_rate.py
use (every log-odds a literal: the format's worst case).  The timed calls do not change the map.  Per map, in ONE loop that alternates
the calls, each timed with the host clock around call + synchronise (median of --reps after --warmup):
  - pack_dev_ms / pack_host_ms:      MLMap.pack into a device tensor / a numpy array (the dry call that sizes included);
  - unpack_dev_ms / unpack_host_ms:  MLMap.unpack of that stream into device tensors / numpy arrays (the sizing call included);
  - save_load_ms:                    MLMap.save to a file and MLMap.load of it into a second handle;
  - numpy_ms, zlib_ms, torch_ms:     the comparators (numpy and zlib --cmp-reps times, without warm-up: seconds per call).
Every pack / unpack row reports the bytes by the rule's own count — pack: 6 read per voxel and 12 per key in each of the two passes, the
stream written; unpack: the stream read twice, 6 written per voxel and 12 per key — and the bytes/s that makes of the median, beside
the HBM peak.  Rows where the call loses are listed under "loses" and printed in bold.  Writes one JSON document.
Usage: python tools/pack_rate.py [--reps 30] [--warmup 2] [--cmp-reps 3] [--out profiles/pack_rate.json]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlmapping_amd import synthetic as syn  # noqa: E402
from mlmapping_amd.config import S1  # noqa: E402
from mlmapping_amd.mlmap import MLMap  # noqa: E402
from tests import delta_ref, pack_ref  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_rate.json"))
    a = ap.parse_args()
    cfg = S1
    C, n_sub = cfg.cells_per_block, cfg.subbox_n
    lo_min, lo_max = np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    out = {"hbm_peak_GBs": HBM_PEAK_GBS, "reps": a.reps, "warmup": a.warmup, "cmp_reps": a.cmp_reps, "maps": {}, "loses": [],
           "not_measured": ["a key box, MLM_PACK_NO_INFL, the rows source", "subbox_n other than 10", "a frontier-mode handle (released blocks are expanded)",
                            "delta(packed=True) and a replica applying it", "calls while frames are in flight (the call drains them first)",
                            "the kernels on their own (host clock around the whole call only)", "a radio link or a disk that is not the page cache"]}
    tmp = tempfile.mkdtemp()

    def raw_export_dev(m, nb):
        t = {"keys": torch.empty((nb, 3), dtype=torch.int32, device="cuda"), "log_odds": torch.empty((nb, C), dtype=torch.float32, device="cuda"),
             "occ": torch.empty((nb, C), dtype=torch.uint8, device="cuda"), "infl": torch.empty((nb, C), dtype=torch.uint8, device="cuda")}
        n_out = ctypes.c_int32()
        m._chk(m._L.mlm_export_blocks(m._h, nb, *[ctypes.c_void_p(t[k].data_ptr()) for k in PLANES], ctypes.byref(n_out)), "mlm_export_blocks")
        return t

    def run_map(tag, m, m2):
        nb = m.block_count()
        path = os.path.join(tmp, tag + ".mlmpack")
        e = m.export_blocks()  # sorted by key: the stream's order
        raw_bytes = nb * (12 + 6 * C)

        def numpy_way():
            t0 = time.perf_counter()
            now = m.export_blocks(raw=True)
            s = pack_ref.pack_map(now, n_sub, lo_min, lo_max)["stream"]
            return (time.perf_counter() - t0) * 1e3, s

        def zlib_way():
            t0 = time.perf_counter()
            now = m.export_blocks(raw=True)
            z = zlib.compress(b"".join(np.ascontiguousarray(now[k]).tobytes() for k in PLANES), 1)
            return (time.perf_counter() - t0) * 1e3, z

        def torch_way():
            sync()
            t0 = time.perf_counter()
            now = raw_export_dev(m, nb)
            flat = now["log_odds"].view(torch.int32).reshape(-1)
            idx = torch.nonzero(flat != 0).reshape(-1)
            vals = flat[idx]
            sync()
            return (time.perf_counter() - t0) * 1e3, (now, idx, vals)

        def timed(fn):
            sync()
            t0 = time.perf_counter()
            r = fn()
            sync()
            return (time.perf_counter() - t0) * 1e3, r

        # every side round-trips the same blocks before anything is timed
        s_host = m.pack()
        s_dev = m.pack(device=True)
        sync()
        summary = [int(v) for v in m.pack_summary]
        assert s_dev.cpu().numpy().tobytes() == s_host.tobytes() == numpy_way()[1], "the call and the numpy encoder differ"
        back = m.unpack(s_host)
        assert all(np.ascontiguousarray(back[k]).tobytes() == np.ascontiguousarray(e[k]).tobytes() for k in PLANES), "unpack(pack()) is not the map"
        z = zlib_way()[1]
        raw_now = m.export_blocks(raw=True)
        assert zlib.decompress(z) == b"".join(np.ascontiguousarray(raw_now[k]).tobytes() for k in PLANES), "zlib does not round-trip"
        now, idx, vals = torch_way()[1]
        again = torch.zeros(nb * C, dtype=torch.int32, device="cuda")
        again[idx] = vals
        assert torch.equal(again, now["log_odds"].view(torch.int32).reshape(-1)), "the compaction does not round-trip"
        o = delta_ref.order(raw_now["keys"])
        assert np.array_equal(raw_now["keys"][o], e["keys"])
        m.save(path)
        m2.load(path)
        e2 = m2.export_blocks()
        assert all(e2[k].tobytes() == e[k].tobytes() for k in PLANES), "save + load is not the map"

        calls = {"pack_dev_ms": lambda: m.pack(device=True), "pack_host_ms": lambda: m.pack(), "unpack_dev_ms": lambda: m.unpack(s_dev, device=True),
                 "unpack_host_ms": lambda: m.unpack(s_host), "save_load_ms": lambda: (m.save(path), m2.load(path))}
        ts = {k: [] for k in list(calls) + ["numpy_ms", "zlib_ms", "torch_ms"]}
        for r in range(a.warmup + a.reps):
            for k, fn in calls.items():
                dt, _ = timed(fn)
                if r >= a.warmup:
                    ts[k].append(dt)
            dt, _ = torch_way()
            if r >= a.warmup:
                ts["torch_ms"].append(dt)
            if len(ts["numpy_ms"]) < a.cmp_reps:  # (in the same loop; seconds per call on the large map, so fewer of them and no warm-up)
                ts["numpy_ms"].append(numpy_way()[0])
                ts["zlib_ms"].append(zlib_way()[0])
        row = {k: stats(v) for k, v in ts.items()}
        stream_bytes = int(s_host.size)
        for k in calls:
            med = row[k]["median"]
            b = {"pack": 2 * nb * (6 * C + 12) + stream_bytes, "unpa": 2 * stream_bytes + nb * (6 * C + 12), "save": None}[k[:4]]
            if b is not None:
                row[k].update(rule_bytes=b, achieved_GBs=b / (med * 1e-3) / 1e9, fraction_of_hbm_peak=b / (med * 1e-3) / 1e9 / HBM_PEAK_GBS)
            if k.startswith("pack"):
                row[k].update(numpy_over_call=row["numpy_ms"]["median"] / med, zlib_over_call=row["zlib_ms"]["median"] / med, torch_over_call=row["torch_ms"]["median"] / med)
        row.update(blocks=nb, raw_bytes=raw_bytes, stream_bytes=stream_bytes, zlib_bytes=len(z), raw_over_stream=raw_bytes / stream_bytes, zlib_over_stream=len(z) / stream_bytes,
                   torch_compaction_bytes=int(idx.numel()) * 8 + 2 * nb * C, summary=summary)
        if len(z) < stream_bytes:
            out["loses"].append(f"{tag}: the stream ({stream_bytes} bytes) is larger than zlib level 1 over the dump ({len(z)} bytes)")
        for k in ("pack_dev_ms", "pack_host_ms"):
            for cmp_k in ("numpy_ms", "zlib_ms", "torch_ms"):
                if row[cmp_k]["median"] < row[k]["median"]:
                    out["loses"].append(f"{tag}: {k} {row[k]['median']:.3f} ms is slower than {cmp_k} {row[cmp_k]['median']:.3f} ms")
        out["maps"][tag].update(row)
        print(tag, json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in row.items() if k != "summary"}), flush=True)

    out["maps"]["corridor"] = {"config": "S1", "scene": "corridor", "frames": 64}
    m = MLMap(cfg, max_blocks=MAX_BLOCKS, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    m2 = MLMap(cfg, max_blocks=MAX_BLOCKS)
    run_map("corridor", m, m2)
    m.close(), m2.close()
    out["maps"]["crafted"] = {"config": "S1", "scene": "32 x 32 x 16 block keys, random planes"}
    big, big2 = MLMap(cfg, max_blocks=4 * MAX_BLOCKS, max_batch=8), MLMap(cfg, max_blocks=4 * MAX_BLOCKS)
    kx, ky, kz = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing="ij")
    keys = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.int32)[rng.permutation(MAX_BLOCKS)]
    big.import_blocks(keys, rng.uniform(-2.0, 4.0, size=(MAX_BLOCKS, C)).astype(np.float32), rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(MAX_BLOCKS, C)),
                      rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(MAX_BLOCKS, C)))
    run_map("crafted", big, big2)
    big.close(), big2.close()
    for line in out["loses"]:
        print("**" + line + "**")
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
