"""Rate of mlm_crop_blocks beside the only way to make a map smaller without it: export_blocks of the whole map to the host, a filter
in numpy, close, a new handle, import_blocks of what is kept.

The map: 64 frames of the S1 corridor stream.  The boxes: a slab across the corridor's long axis that holds about 10 % and about 50 %
of the blocks, dropped with MLM_CROP_INSIDE (a window rolling forward drops what lies behind).  Device in, device out.  Per box, in
ONE loop that alternates the calls, each timed with the host clock around call + synchronise; before every timed call the handle is
put back (not timed): everything dropped, the snapshot of the whole map imported from device memory.
  - crop_ms:          no outputs: the blocks are just dropped;
  - crop_page_dev_ms: page-out of the five arrays into device memory;
  - crop_page_pin_ms: page-out into pinned host memory (staged);
  - crop_dry_ms:      MLM_CROP_DRY, the count alone;
  - crop_shrink_ms:   no outputs, MLM_CROP_SHRINK (the 50 % box only), on a second handle with the same map whose pool started at 64
                      blocks and grew on the way, so that the pool really moves into a smaller one; its bytes include that copy;
  - rebuild_ms / rebuild_no_create_ms: the comparator, with and without the creation of the new handle in the clock.
Before anything is timed the comparator's new handle and the cropped handle must hold the same map (their sorted exports are compared).
Every crop row reports the bytes the rule says must move — computed here from D, H and the cells of a block: a pair of the move reads
and writes a block's key and planes, the page-out reads and writes a dropped block and its flag, the tail reset writes the planes and
the per-voxel scratch of D slots — and the bytes/s that makes of the median, beside the HBM peak.  The corridor map is a megabyte, so
its rows are latency; the same rows (a third of the repetitions, no SHRINK row) are taken on a crafted map of 16 384 blocks as well.
Writes one JSON document.  Usage: python tools/crop_rate.py [--reps 30] [--warmup 2] [--out profiles/crop_rate.json]"""
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

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
KEY_MIN = -(1 << 20)
WHOLE = ([KEY_MIN] * 3, [1 << 21] * 3)
MAX_BLOCKS = 16384


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def build(cfg, max_blocks=MAX_BLOCKS):
    m = MLMap(cfg, max_blocks=max_blocks, max_batch=8)
    frames = list(syn.stream(cfg, "corridor", "smooth", 64))
    for k0 in range(0, 64, 8):
        fr = frames[k0:k0 + 8]
        m.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1][0] for f in fr]), np.stack([f[1][1] for f in fr]))
    m.sync()
    return m


def slab(keys, fraction):
    """INSIDE box along the axis of greatest extent that holds about `fraction` of the blocks (those with the lowest keys)"""
    k = keys.astype(np.int64)
    ax = int(np.argmax(k.max(0) - k.min(0)))
    cut = int(np.sort(k[:, ax])[max(1, int(round(fraction * len(k)))) - 1]) + 1
    lo, dims = [KEY_MIN] * 3, [1 << 21] * 3
    dims[ax] = cut - KEY_MIN
    return lo, dims


def drops(keys, lo, dims):
    k = keys.astype(np.int64)
    return ((k >= np.array(lo)) & (k < np.array(lo) + np.array(dims))).all(axis=1)


def rule_bytes(drop, cells, page, frontier=False):
    """D, H and the bytes the rule moves for these drop flags (raw slot order)"""
    nb, D = len(drop), int(drop.sum())
    K = nb - D
    H = int(drop[:K].sum())
    block = 12 + 6 * cells + ((cells + 2) if frontier else 0)
    move = 2 * H * block
    page_out = 2 * D * (block + 1) if page else 0
    tail = D * cells * (6 + 16 + (9 if frontier else 0))
    return {"D": D, "K": K, "H": H, "move_bytes": move, "page_bytes": page_out, "tail_reset_bytes": tail, "bytes": move + page_out + tail}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "crop_rate.json"))
    a = ap.parse_args()
    cfg = S1
    C = cfg.cells_per_block
    sync = torch.cuda.synchronize
    out = {"hbm_peak_GBs": HBM_PEAK_GBS, "reps": a.reps, "warmup": a.warmup, "maps": {}, "cases": {},
           "not_measured": ["frontier-mode handles", "subbox_n other than 10", "page-out into pageable host memory", "a shrink that fails for lack of memory"]}

    def run_map(tag, m, grown, fractions, reps):
        """every row for the map handle m holds; `grown`: a handle with the same map whose pool started at 64 blocks (the SHRINK row)"""
        whole = m.export_blocks()
        nb = len(whole["keys"])
        out["maps"][tag]["blocks"], out["maps"][tag]["cells"], out["maps"][tag]["map_bytes"] = nb, C, nb * (12 + 6 * C)
        snap = {k: torch.from_numpy(whole[k]).cuda() for k in ("keys", "log_odds", "occ", "infl")}
        dev = {"keys": torch.empty((nb, 3), dtype=torch.int32, device="cuda"), "log_odds": torch.empty((nb, C), dtype=torch.float32, device="cuda"),
               "occ": torch.empty((nb, C), dtype=torch.uint8, device="cuda"), "infl": torch.empty((nb, C), dtype=torch.uint8, device="cuda"),
               "collapsed": torch.empty(nb, dtype=torch.uint8, device="cuda")}
        pin = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in dev.items()}
        sync()

        def restore(h):
            h.crop_blocks(*WHOLE, inside=True)
            h.import_blocks((snap["keys"].data_ptr(), nb), snap["log_odds"].data_ptr(), snap["occ"].data_ptr(), snap["infl"].data_ptr())

        def rebuild(lo, dims, timed_create):
            """the comparator; returns (milliseconds, the new handle)"""
            t0 = time.perf_counter()
            b = m.export_blocks(raw=True)
            keep = ~drops(b["keys"], lo, dims)
            kept = {k: np.ascontiguousarray(v[keep]) for k, v in b.items()}
            t1 = time.perf_counter()
            new = MLMap(cfg, max_blocks=MAX_BLOCKS, max_batch=8)  # (the old handle is closed by the caller: the tool still needs it)
            t2 = time.perf_counter()
            new.import_blocks(kept["keys"], kept["log_odds"], kept["occ"], kept["infl"])
            sync()
            t3 = time.perf_counter()
            return ((t3 - t0) if timed_create else (t1 - t0) + (t3 - t2)) * 1e3, new

        for name, fraction in fractions:
            lo, dims = slab(whole["keys"], fraction)
            variants = {
                "crop_ms": (m, dict()),
                "crop_page_dev_ms": (m, dict(out={"cap": nb, **{k: v.data_ptr() for k, v in dev.items()}})),
                "crop_page_pin_ms": (m, dict(out={"cap": nb, **{k: v.data_ptr() for k, v in pin.items()}})),
                "crop_dry_ms": (m, dict(dry=True)),
            }
            if grown is not None and fraction >= 0.5:
                variants["crop_shrink_ms"] = (grown, dict(shrink=True))
            # the same map on both sides before anything is timed
            restore(m)
            _, new = rebuild(lo, dims, True)
            m.crop_blocks(lo, dims, inside=True)
            g, c = m.export_blocks(), new.export_blocks()
            assert all(np.array_equal(g[k].view(np.uint8), c[k].view(np.uint8)) for k in ("keys", "log_odds", "occ", "infl")), "the comparator holds another map"
            new.close()
            ts = {k: [] for k in list(variants) + ["rebuild_ms", "rebuild_no_create_ms"]}
            rule = {k: [] for k in variants}
            summaries = {}
            for r in range(a.warmup + reps):
                for k, (h, kw) in variants.items():  # (alternating: the calls see the same machine)
                    restore(h)
                    drop = drops(h.export_blocks(raw=True)["keys"], lo, dims)
                    sync()
                    t0 = time.perf_counter()
                    res = h.crop_blocks(lo, dims, inside=True, **kw)
                    sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    if r >= a.warmup:
                        ts[k].append(dt)
                        rule[k].append(rule_bytes(drop, C, page="out" in kw))
                        summaries[k] = [int(v) for v in res["summary"]]
                restore(m)
                for k, timed_create in (("rebuild_ms", True), ("rebuild_no_create_ms", False)):
                    dt, new = rebuild(lo, dims, timed_create)
                    new.close()
                    if r >= a.warmup:
                        ts[k].append(dt)
            row = {k: stats(v) for k, v in ts.items()}
            for k in variants:
                med = row[k]["median"]
                b = {f: float(np.median([x[f] for x in rule[k]])) for f in rule[k][0]}
                if k == "crop_dry_ms":
                    b["move_bytes"] = b["tail_reset_bytes"] = b["bytes"] = 0.0
                if k == "crop_shrink_ms":  # (the K kept blocks are read and written once more, into the smaller pool)
                    b["shrink_copy_bytes"] = 2.0 * b["K"] * (12 + 6 * C)
                    b["bytes"] += b["shrink_copy_bytes"]
                row[k].update(rule=b, summary=summaries[k], achieved_GBs=b["bytes"] / (med * 1e-3) / 1e9,
                              fraction_of_hbm_peak=b["bytes"] / (med * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              rebuild_over_call=row["rebuild_ms"]["median"] / med, rebuild_no_create_over_call=row["rebuild_no_create_ms"]["median"] / med)
            row.update(key_lo=[int(v) for v in lo], key_dims=[int(v) for v in dims], reps=reps)
            out["cases"][f"{tag}_{name}"] = row

    # the corridor map after 64 frames; for the SHRINK row a handle whose pool started small and grew on the way
    out["maps"]["corridor"] = {"config": "S1", "scene": "corridor", "frames": 64}
    m, grown = build(cfg), build(cfg, 64)
    run_map("corridor", m, grown, (("drop10", 0.10), ("drop50", 0.50)), a.reps)
    m.close(), grown.close()
    # beyond the corridor (which is a megabyte: the rows above are latency): a crafted map of 16 384 blocks, 98 MB of planes
    out["maps"]["crafted"] = {"config": "S1", "scene": "32 x 32 x 16 block keys, random planes"}
    big = MLMap(cfg, max_blocks=2 * MAX_BLOCKS, max_batch=8)
    rng = np.random.default_rng(0)
    kx, ky, kz = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing="ij")
    keys = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.int32)[rng.permutation(MAX_BLOCKS)]
    big.import_blocks(keys, rng.uniform(-2, 4, size=(MAX_BLOCKS, C)).astype(np.float32), rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(MAX_BLOCKS, C)),
                      rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(MAX_BLOCKS, C)))
    run_map("crafted", big, None, (("drop10", 0.10), ("drop50", 0.50)), max(3, a.reps // 3))
    big.close()
    doc = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
