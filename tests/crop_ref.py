"""The rule of mlm_crop_blocks (include/mlmap_hip.h, mlmapping_amd/csrc/mlm_crop.h) in numpy, written from the contract: the argument
check, the predicate, the hole-filling compaction, the output rows, the summary's counts and the shrink rule.  The CPU driver
(tests/cpp/crop_driver.cpp, the header's own code in the device's phase order) and the GPU (tests/test_gpu_crop.py) are held to it."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
OUTSIDE, INSIDE, DRY, SHRINK, ROW = 0, 1, 2, 4, 8
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3
KEY_MIN, KEY_MAX = -(1 << 20), (1 << 20) - 1  # both ends of the 21-bit key range


def check_args(key_lo, key_dims, flags, cap):
    """0: fine; 1: no box; 2: a dim < 1; 3: key_lo + key_dims beyond int32; 4: an unknown flag bit; 5: cap < 0"""
    if key_lo is None or key_dims is None:
        return 1
    if any(int(d) < 1 for d in key_dims):
        return 2
    if any(int(l) + int(d) > I32_MAX for l, d in zip(key_lo, key_dims)):
        return 3
    if flags & ~(INSIDE | DRY | SHRINK):
        return 4
    if cap < 0:
        return 5
    return 0


def drops(keys, key_lo, key_dims, inside):
    """which blocks the box drops: bool [n]"""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    lo = np.asarray(key_lo, dtype=np.int64)
    hi = lo + np.asarray(key_dims, dtype=np.int64)
    within = ((k >= lo) & (k < hi)).all(axis=1)
    return within if inside else ~within


def plan(drop):
    """D, K, H, `rows` (old slots of the dropped blocks in output order) and `order` (order[i] = the old slot whose block is in slot i
    afterwards, i < K): the dropped slot below K with h dropped slots below it takes the h-th kept slot at or above K"""
    drop = np.asarray(drop, dtype=bool)
    nb = len(drop)
    rows = np.flatnonzero(drop)
    D = len(rows)
    K = nb - D
    holes = rows[rows < K]
    fillers = np.flatnonzero(~drop)
    fillers = fillers[fillers >= K]
    assert len(holes) == len(fillers)
    order = np.arange(K)
    order[holes] = fillers
    return {"D": D, "K": K, "H": len(holes), "rows": rows, "order": order}


def crop(blocks, key_lo, key_dims, inside):
    """blocks: {"keys", "log_odds", "occ", "infl"[, "collapsed"]} in raw slot order -> (the kept blocks in the raw order after the call,
    the dropped blocks in output order, the plan)"""
    p = plan(drops(blocks["keys"], key_lo, key_dims, inside))
    kept = {k: np.asarray(v)[p["order"]] for k, v in blocks.items()}
    out = {k: np.asarray(v)[p["rows"]] for k, v in blocks.items()}
    return kept, out, p


def shrink_target(c0, capacity, K):
    """the capacity MLM_CROP_SHRINK moves the pool to, or 0: the smallest c0 * 2^k >= max(c0, 2 K), if that is below the capacity"""
    t = c0
    while t < max(c0, 2 * K):
        t *= 2
    return t if t < capacity else 0


def retain_box(t_w, radius, d_glb):
    """retain_around's key box: floor((t - r) / d_glb) - 1 .. floor((t + r) / d_glb) + 1 per axis, as (key_lo, key_dims)"""
    t = np.asarray(t_w, dtype=np.float64)
    lo = np.floor((t - radius) / d_glb).astype(np.int64) - 1
    hi = np.floor((t + radius) / d_glb).astype(np.int64) + 1
    return lo, hi - lo + 1
