"""The contract of mlm_delta_blocks (include/mlmap_hip.h) in numpy: the argument check with its codes, the selection, the view of a
block, the digest, the join against a previous table, the order of the tables, the emitted blocks and the gone keys, the summary and the
capacity rule.  Written from the header's text, apart from mlmapping_amd/csrc/mlm_delta.h: the join is a dictionary lookup, not a
binary search, and the order is a lexsort of the keys, not a sort of packed words."""
import numpy as np

from tests import crop_ref

DRY, NO_INFL, ALL_FLAGS = 1, 2, 3
ROW = 12
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3
UNCHANGED, CHANGED, NEW = 0, 1, 2
U, F, O = ord("u"), ord("f"), ord("o")
KEY_MIN, KEY_MAX = -(1 << 20), (1 << 20) - 1
GOLD, SECOND = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
BLANK8 = (0xaa5d834bd09a229e, 0x71cf1fe0a9b5a6df)  # the digest of the all-blank block of 8 cells (0.0f / 'u' / 'u')
TEXTS = {1: "key_lo and key_dims must be given together", 2: "key_dims must be >= 1", 3: "key_lo + key_dims must fit an int32", 4: "unknown flag bit",
         5: "cap_table, cap, cap_gone and n_prev must be >= 0", 6: "n_prev > 0 takes prev_keys and prev_digest",
         7: "a previous key lies outside the 21-bit key range", 8: "the previous keys must be strictly ascending by packed key"}


def pack(keys):
    """the packed key: x, then y, then z, each biased by 2^20 (21 bits each)"""
    k = (np.asarray(keys, dtype=np.int64).reshape(-1, 3) + (1 << 20)) & 0x1FFFFF
    return (k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64)


def order(keys):
    keys = np.asarray(keys).reshape(-1, 3)
    return np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))


def mix(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * M1
        x = x ^ (x >> np.uint64(27))
        x = x * M2
        return x ^ (x >> np.uint64(31))


def digest(log_odds, occ, infl):
    """uint64 [blocks, 2] of planes [blocks, cells]"""
    lo = np.ascontiguousarray(log_odds, dtype=np.float32)
    nb = lo.shape[0]
    C = lo.shape[1] if lo.ndim == 2 else 0
    w = lo.view(np.uint32).astype(np.uint64).reshape(nb, C) | (np.asarray(occ, dtype=np.uint8).reshape(nb, C).astype(np.uint64) << np.uint64(32)) | \
        (np.asarray(infl, dtype=np.uint8).reshape(nb, C).astype(np.uint64) << np.uint64(40))
    with np.errstate(over="ignore"):
        x = w ^ ((np.arange(C, dtype=np.uint64) + np.uint64(1)) * GOLD)[None, :]
        d0 = mix(x).sum(axis=1, dtype=np.uint64)
        d1 = mix(x ^ SECOND).sum(axis=1, dtype=np.uint64)
    return np.stack([d0, d1], axis=1).reshape(nb, 2)


def view(b, no_infl=False):
    """the planes the call reads: a released block answers from element 0 with infl 'u'; with no_infl infl is 'u' everywhere"""
    lo = np.array(b["log_odds"], dtype=np.float32, copy=True)
    occ, infl = np.array(b["occ"], dtype=np.uint8, copy=True), np.array(b["infl"], dtype=np.uint8, copy=True)
    col = np.asarray(b.get("collapsed", np.zeros(len(lo), dtype=np.uint8))).astype(bool).reshape(len(lo))
    if col.any():
        lo[col] = lo[col][:, :1]
        occ[col] = occ[col][:, :1]
        infl[col] = U
    if no_infl:
        infl[:] = U
    return lo, occ, infl


def check_args(key_lo, key_dims, n_prev, has_prev, flags, cap_table=0, cap=0, cap_gone=0):
    """0: fine; 1: one of key_lo / key_dims missing; 2: a dim < 1; 3: key_lo + key_dims beyond int32; 4: an unknown flag bit; 5: a negative
    cap or n_prev; 6: n_prev > 0 without a table.  (7: a previous key out of range and 8: keys not strictly ascending: check_prev)"""
    if (key_lo is None) != (key_dims is None):
        return 1
    if key_lo is not None:
        bad = crop_ref.check_args(key_lo, key_dims, 0, 0)
        if bad:
            return bad
    if flags & ~ALL_FLAGS:
        return 4
    if min(cap_table, cap, cap_gone, n_prev) < 0:
        return 5
    if n_prev > 0 and not has_prev:
        return 6
    return 0


def check_prev(prev_keys):
    k = np.asarray(prev_keys, dtype=np.int64).reshape(-1, 3)
    if ((k < KEY_MIN) | (k > KEY_MAX)).any():
        return 7
    p = pack(k)
    if len(p) > 1 and (p[1:] <= p[:-1]).any():
        return 8
    return 0


def in_box(keys, key_lo, key_dims):
    keys = np.asarray(keys).reshape(-1, 3)
    if key_lo is None:
        return np.ones(len(keys), dtype=bool)
    return crop_ref.drops(keys, key_lo, key_dims, inside=True)


def empty_blocks(b):
    """mlm_age_blocks' EMPTY predicate on the planes as they are (a released block: element 0, infl 'u')"""
    lo, occ, infl = view(b)
    ev = (lo.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0
    return ((occ == U) & (infl != O) & ~ev).all(axis=1)


def delta(b, prev=None, key_lo=None, key_dims=None, no_infl=False):
    """the full answer of a call with room for everything: a dict with "status", "code", and — status OK — "table" (keys int32 [S, 3],
    digest uint64 [S, 2]), "keys", "log_odds", "occ", "infl", "kind" of the emitted blocks, "gone" int32 [G, 3], "summary" int64 [12]
    with [8] .. [10] as a call that writes everything reports them.  prev: (keys, digest) or None."""
    keys = np.asarray(b["keys"], dtype=np.int32).reshape(-1, 3)
    nb = len(keys)
    pk = np.zeros((0, 3), dtype=np.int32) if prev is None else np.asarray(prev[0], dtype=np.int32).reshape(-1, 3)
    pd = np.zeros((0, 2), dtype=np.uint64) if prev is None else np.asarray(prev[1], dtype=np.uint64).reshape(-1, 2)
    code = check_args(key_lo, key_dims, len(pk), True, NO_INFL if no_infl else 0) or check_prev(pk)
    if code:
        return {"status": ERR_INVALID, "code": code, "text": TEXTS[code]}
    lo, occ, infl = view(b, no_infl)
    C = lo.shape[1] if lo.ndim == 2 else 0
    sel = np.nonzero(in_box(keys, key_lo, key_dims))[0]
    sel = sel[order(keys[sel])]
    dg = digest(lo[sel], occ[sel], infl[sel]) if len(sel) else np.zeros((0, 2), dtype=np.uint64)
    pin = in_box(pk, key_lo, key_dims)
    before = {tuple(k): tuple(int(x) for x in d) for k, d, i in zip(pk.tolist(), pd, pin) if i}
    kind = np.array([NEW if tuple(k) not in before else UNCHANGED if before[tuple(k)] == tuple(int(x) for x in d) else CHANGED
                     for k, d in zip(keys[sel].tolist(), dg)], dtype=np.uint8).reshape(len(sel))
    held = {tuple(k) for k in keys[sel].tolist()}
    gone = np.array([k for k, i in zip(pk.tolist(), pin) if i and tuple(k) not in held], dtype=np.int32).reshape(-1, 3)
    gone = gone[order(gone)]
    em = sel[kind != UNCHANGED]
    n_unch, n_ch, n_new = (int((kind == v).sum()) for v in (UNCHANGED, CHANGED, NEW))
    n_empty = int(empty_blocks({k: np.asarray(v)[sel] for k, v in b.items()}).sum()) if len(sel) else 0
    summary = np.array([nb, len(sel), len(pk), int(pin.sum()), n_unch, n_ch, n_new, len(gone), len(em), len(sel), len(gone), n_empty], dtype=np.int64)
    assert summary[1] == n_unch + n_ch + n_new and summary[3] == n_unch + n_ch + len(gone)
    return {"status": OK, "code": 0, "table": (keys[sel].reshape(-1, 3), dg.reshape(-1, 2)), "keys": keys[em].reshape(-1, 3), "log_odds": lo[em].reshape(-1, C),
            "occ": occ[em].reshape(-1, C), "infl": infl[em].reshape(-1, C), "kind": kind[kind != UNCHANGED], "gone": gone, "summary": summary}


def capacity_short(summary, cap_table, cap, cap_gone, table_out=True, block_out=True, gone_out=True):
    """does the call answer MLM_ERR_CAPACITY?  (a cap counts only where one of its outputs is given)"""
    return bool((table_out and cap_table < summary[1]) or (block_out and cap < summary[5] + summary[6]) or (gone_out and cap_gone < summary[7]))


def apply(b, d):
    """a replica's map after it took the delta: emitted blocks overwrite or join, gone keys leave; sorted by key"""
    at = {tuple(k): i for i, k in enumerate(np.asarray(b["keys"]).reshape(-1, 3).tolist())}
    rows = {k: (b["log_odds"][i], b["occ"][i], b["infl"][i]) for k, i in at.items()}
    for i, k in enumerate(d["keys"].tolist()):
        rows[tuple(k)] = (d["log_odds"][i], d["occ"][i], d["infl"][i])
    for k in d["gone"].tolist():
        rows.pop(tuple(k), None)
    ks = sorted(rows, key=lambda k: (k[0], k[1], k[2]))
    C = d["log_odds"].shape[1]
    return {"keys": np.array(ks, dtype=np.int32).reshape(-1, 3), "log_odds": np.array([rows[k][0] for k in ks], dtype=np.float32).reshape(-1, C),
            "occ": np.array([rows[k][1] for k in ks], dtype=np.uint8).reshape(-1, C), "infl": np.array([rows[k][2] for k in ks], dtype=np.uint8).reshape(-1, C)}
