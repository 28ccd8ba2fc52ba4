"""The contract of mlm_fuse_blocks (include/mlmap_hip.h) in numpy: the argument check with its codes, the key checks, and the fuse of a
block dump into a map given in raw slot order — the map afterwards in raw slot order, the summary and per_row.  Written from the
header's text, apart from mlmapping_amd/csrc/mlm_fuse.h: the counts are taken from the planes before and after, not from event bits."""
import numpy as np

ADD, MAX, TAKE, FILL = 0, 1, 2, 3
MODES = {"add": ADD, "max": MAX, "take": TAKE, "fill": FILL}
DRY, ROW, COLS = 1, 12, 4
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3
U, F, O = ord("u"), ord("f"), ord("o")
KEY_MIN, KEY_MAX = -(1 << 20), (1 << 20) - 1
LIMITS = (-2.0, 4.2, 2.0)  # log_odds_min, log_odds_max, occupied_sh of the S1 configuration


def check_args(n, keys, log_odds, occ, mode, flags):
    """0: fine; 1: n < 0; 2: keys, log_odds or occ missing with n > 0; 3: mode outside 0..3; 4: an unknown flag bit"""
    if n < 0:
        return 1
    if n > 0 and (keys is None or log_odds is None or occ is None):
        return 2
    if not 0 <= mode <= 3:
        return 3
    if flags & ~DRY:
        return 4
    return 0


def check_keys(keys):
    """0: fine; 5: a key outside the 21-bit range; 6: two rows with the same key"""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    if ((k < KEY_MIN) | (k > KEY_MAX)).any():
        return 5
    if len({tuple(r) for r in k.tolist()}) != len(k):
        return 6
    return 0


def clamp(x, lim):
    lo_min, lo_max = np.float32(lim[0]), np.float32(lim[1])
    with np.errstate(invalid="ignore"):
        return np.where(~(x >= lo_min), lo_min, np.where(x > lo_max, lo_max, x)).astype(np.float32)


def expanded(blocks):
    """a frontier-mode export as k_merge_pack and the queries read it: a released block answers from element 0 with infl 'u'"""
    out = {k: np.array(v, copy=True) for k, v in blocks.items()}
    col = np.asarray(blocks.get("collapsed", np.zeros(len(blocks["keys"]), np.uint8))).astype(bool)
    for k in ("log_odds", "occ"):
        out[k][col] = out[k][col][:, :1]
    out["infl"][col] = U
    return out


def fuse(map_blocks_raw, rows, mode, dry=False, infl_given=True, lim=LIMITS):
    """(map afterwards in raw slot order, summary int64 [12], per_row int32 [n, 4]); the inputs are not changed.  With dry the map
    returned is the map given."""
    mode = MODES.get(mode, mode)
    m = {k: np.array(map_blocks_raw[k], copy=True) for k in ("keys", "log_odds", "occ", "infl")}
    nb, C = m["log_odds"].shape
    keys = np.asarray(rows["keys"], dtype=np.int32).reshape(-1, 3)
    n = len(keys)
    Lb = np.asarray(rows["log_odds"], dtype=np.float32).reshape(n, C)
    ob = np.asarray(rows["occ"], dtype=np.uint8).reshape(n, C)
    ib = np.asarray(rows["infl"], dtype=np.uint8).reshape(n, C) if infl_given else np.full((n, C), U, dtype=np.uint8)
    assert check_keys(keys) == 0
    slot_of = {tuple(k): s for s, k in enumerate(m["keys"].tolist())}
    slot = np.array([slot_of.get(tuple(k), -1) for k in keys.tolist()], dtype=np.int64)
    contrib = (ob == F) | (ob == O)
    touch = contrib.any(axis=1) | (ib == O).any(axis=1)
    created = (slot < 0) & touch
    new_slot = np.where(created, nb + np.cumsum(created) - created, slot)
    n_new = int(created.sum())
    # the map's side of every row: what it holds, or 0.0f / 'u' / 'u'
    have = slot >= 0
    La = np.zeros((n, C), dtype=np.float32)
    oa = np.full((n, C), U, dtype=np.uint8)
    ia = np.full((n, C), U, dtype=np.uint8)
    La[have], oa[have], ia[have] = m["log_odds"][slot[have]], m["occ"][slot[have]], m["infl"][slot[have]]
    seen_a = oa != U
    Lc = clamp(Lb, lim)
    with np.errstate(invalid="ignore", over="ignore"):
        L = La + Lc if mode == ADD else np.where(seen_a, np.where(La > Lc, La, Lc), Lc) if mode == MAX else Lc
        L = clamp(L.astype(np.float32), lim)
    written = contrib & (~seen_a if mode == FILL else True)
    La2 = np.where(written, L, La).astype(np.float32)
    oa2 = np.where(written, np.where(L > np.float32(lim[2]), O, F), oa).astype(np.uint8)
    ia2 = np.where(ib == O, O, ia).astype(np.uint8)
    to_o, o_to_f = (oa2 == O) & (oa != O), (oa == O) & (oa2 == F)
    conflict = contrib & seen_a & (oa != ob)
    summary = np.array([n, int(have.sum()), n_new, int((~touch).sum()), int(contrib.sum()), int((contrib & ~seen_a).sum()),
                        int((contrib & seen_a & (oa == ob)).sum()), int(conflict.sum()), int(to_o.sum()), int(o_to_f.sum()),
                        int(((ia2 == O) & (ia != O)).sum()), int((La2.view(np.uint32) != La.view(np.uint32)).sum())], dtype=np.int64)
    per_row = np.stack([contrib.sum(axis=1), conflict.sum(axis=1), (to_o | o_to_f).sum(axis=1), np.where(have, 0, np.where(created, 1, 2))],
                       axis=1).astype(np.int32).reshape(n, COLS)
    if not dry:
        grow = lambda a, fill: np.concatenate([a, np.full((n_new,) + a.shape[1:], fill, dtype=a.dtype)])
        m = {"keys": grow(m["keys"], 0), "log_odds": grow(m["log_odds"], 0), "occ": grow(m["occ"], U), "infl": grow(m["infl"], U)}
        m["keys"][new_slot[created]] = keys[created]
        t = touch  # (a row that touches nothing changes nothing; an absent one has no slot)
        m["log_odds"][new_slot[t]], m["occ"][new_slot[t]], m["infl"][new_slot[t]] = La2[t], oa2[t], ia2[t]
    return m, summary, per_row


def sorted_blocks(b):
    o = np.lexsort((b["keys"][:, 2], b["keys"][:, 1], b["keys"][:, 0]))
    return {k: np.asarray(v)[o] for k, v in b.items()}
