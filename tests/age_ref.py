"""The contract of mlm_age_blocks (include/mlmap_hip.h) in numpy: the argument check with its codes, the selection, the per-voxel rule, the
empty-block predicate and the drop by mlm_crop_blocks' hole filling (tests/crop_ref.py) — the map afterwards in raw slot order, the
summary and per_block.  Written from the header's text, apart from mlmapping_amd/csrc/mlm_age.h: the counts are taken from the planes
before and after, not from event bits.  Float32 throughout."""
import numpy as np

from tests import crop_ref

SCALE, STEP = 0, 1
MODES = {"scale": SCALE, "step": STEP}
OUTSIDE, DRY, FORGET, DROP, CLEAR_INFL, ALL_FLAGS = 1, 2, 4, 8, 16, 31
ROW, COLS = 12, 4
OK, ERR_INVALID = 0, -1
U, F, O = ord("u"), ord("f"), ord("o")
LIMITS = (-2.0, 4.2, 2.0)  # log_odds_min, log_odds_max, occupied_sh of the S1 configuration
TEXTS = {1: "key_lo and key_dims must be given together", 2: "key_dims must be >= 1", 3: "key_lo + key_dims must fit an int32", 4: "unknown flag bit",
         5: "mode must be MLM_AGE_SCALE or MLM_AGE_STEP", 6: "amount must be finite", 7: "MLM_AGE_SCALE takes an amount in [0, 1]",
         8: "MLM_AGE_STEP takes an amount >= 0", 9: "MLM_AGE_FORGET takes a finite forget >= 0"}


def check_args(key_lo, key_dims, mode, amount, forget, flags):
    """0: fine; 1: one of key_lo / key_dims missing; 2: a dim < 1; 3: key_lo + key_dims beyond int32; 4: an unknown flag bit; 5: a mode
    outside 0..1; 6: a non-finite amount; 7: SCALE with amount outside [0, 1]; 8: STEP with amount < 0; 9: FORGET with a non-finite or
    negative forget"""
    if (key_lo is None) != (key_dims is None):
        return 1
    if key_lo is not None:
        bad = crop_ref.check_args(key_lo, key_dims, 0, 0)
        if bad:
            return bad
    if flags & ~ALL_FLAGS:
        return 4
    if mode not in (SCALE, STEP):
        return 5
    amount, forget = np.float32(amount), np.float32(forget)
    if not np.isfinite(amount):
        return 6
    if mode == SCALE and not (amount >= 0 and amount <= 1):
        return 7
    if mode == STEP and amount < 0:
        return 8
    if (flags & FORGET) and (not np.isfinite(forget) or forget < 0):
        return 9
    return 0


def clamp(x, lim):
    lo_min, lo_max = np.float32(lim[0]), np.float32(lim[1])
    with np.errstate(invalid="ignore"):
        return np.where(~(x >= lo_min), lo_min, np.where(x > lo_max, lo_max, x)).astype(np.float32)


def selected(keys, key_lo, key_dims, outside):
    """which blocks the call selects: bool [n]"""
    keys = np.asarray(keys).reshape(-1, 3)
    if key_lo is None:
        return np.ones(len(keys), dtype=bool)
    return crop_ref.drops(keys, key_lo, key_dims, inside=not outside)


def has_evidence(lo):
    return (np.ascontiguousarray(lo, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0


def empty_blocks(b):
    """the EMPTY predicate per block: every voxel occ 'u', infl other than 'o', log-odds +-0.0f"""
    return ((b["occ"] == U) & (b["infl"] != O) & ~has_evidence(b["log_odds"])).all(axis=1)


def age(map_blocks_raw, key_lo=None, key_dims=None, mode=SCALE, amount=1.0, forget=None, outside=False, drop=False, clear_infl=False, dry=False,
        lim=LIMITS):
    """(map afterwards in raw slot order, summary int64 [12], per_block int32 [blocks before, 4]); the inputs are not changed.  With dry
    the map returned is the map given."""
    mode = MODES.get(mode, mode)
    m = {k: np.array(map_blocks_raw[k], copy=True) for k in ("keys", "log_odds", "occ", "infl")}
    nb = len(m["keys"])
    C = m["log_odds"].shape[1] if m["log_odds"].ndim == 2 else 0
    La, oa, ia = m["log_odds"].astype(np.float32).reshape(nb, C), m["occ"].reshape(nb, C), m["infl"].reshape(nb, C)
    sel = selected(m["keys"], key_lo, key_dims, outside)
    amount = np.float32(amount)
    aged = sel[:, None] & ((oa != U) | has_evidence(La))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if mode == SCALE:
            L = (La * amount).astype(np.float32)
        else:
            L = np.where(La > amount, La - amount, np.where(La < -amount, La + amount, np.float32(0.0))).astype(np.float32)
        L = clamp(L, lim)
        forgot = aged & (np.abs(L) <= np.float32(forget)) if forget is not None else np.zeros_like(aged)
    La2 = np.where(aged, np.where(forgot, np.float32(0.0), L), La).astype(np.float32)
    cls = np.where(L > np.float32(lim[2]), O, F).astype(np.uint8)
    oa2 = np.where(forgot, U, np.where(aged & (oa != U), cls, oa)).astype(np.uint8)
    ia2 = np.where(sel[:, None], U, ia).astype(np.uint8) if clear_infl else ia.copy()
    after = {"keys": m["keys"], "log_odds": La2, "occ": oa2, "infl": ia2}
    empty = sel & empty_blocks(after) if nb else np.zeros(0, dtype=bool)
    o_to_f, f_to_o = (oa == O) & (oa2 == F), (oa == F) & (oa2 == O)
    n_drop = int(empty.sum()) if drop else 0
    summary = np.array([nb, int(sel.sum()), n_drop, nb - n_drop, int(aged.sum()), int((La2.view(np.uint32) != La.view(np.uint32)).sum()), int(forgot.sum()),
                        int((forgot & (oa == O)).sum()), int((forgot & (oa == F)).sum()), int(o_to_f.sum()), int(f_to_o.sum()),
                        int(((ia == O) & (ia2 == U)).sum())], dtype=np.int64)
    per_block = np.stack([aged.sum(axis=1), forgot.sum(axis=1), (o_to_f | f_to_o).sum(axis=1), np.where(sel, np.where(empty, 2, 1), 0)],
                         axis=1).astype(np.int32).reshape(nb, COLS)
    if dry:
        return m, summary, per_block
    if drop and n_drop:
        order = crop_ref.plan(empty)["order"]
        after = {k: v[order] for k, v in after.items()}
    return after, summary, per_block


def sorted_blocks(b):
    o = np.lexsort((b["keys"][:, 2], b["keys"][:, 1], b["keys"][:, 0]))
    return {k: np.asarray(v)[o] for k, v in b.items()}
