"""The contract of mlm_warp_blocks (include/mlmap_hip.h, mlmapping_amd/csrc/mlm_warp.h) in numpy, brute force and written from the contract:
the argument check, the gather per destination voxel, the live predicate, the emitted blocks in ascending key order and the summary's
counts.  It uses no part of the library.  The CPU driver (tests/cpp/warp_driver.cpp, the header's own code in the device's phase order)
and the GPU (tests/test_gpu_warp.py) are held to it byte for byte.

Per destination voxel v = g * n + c, in float64, elementwise, the same five operations per axis in the same order:
    p_a = (g_a * d_glb + c_a * d_sub) + d_sub_half
    w_a = ((R[a][0] * p_0 + R[a][1] * p_1) + R[a][2] * p_2) + o_a
    Q_a = floor((w_a / d_sub) * 1024.0), invalid unless |Q_a| < 2^40;  source voxel Q_a // 1024, block and cell by floor division.
Which destination blocks are looked at: for every source block the keys its eight corners reach under the inverse transform, two blocks
more on every side (far more than the library's one voxel: every block with a live voxel is among them)."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SEEN, REPLACE, DRY, ROW = 1, 2, 4, 8
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3
KEY_MIN, KEY_MAX = -(1 << 20), (1 << 20) - 1  # both ends of the 21-bit key range
RIGID_TOL = 1e-9
U, O, F = ord("u"), ord("o"), ord("f")


def check_args(T, key_lo, key_dims, flags, cap):
    """0: fine; 1: no transform; 2: a non-finite entry; 3: not rigid; 4: one of key_lo / key_dims missing; 5: a key dim < 1;
    6: key_lo + key_dims beyond int32; 7: an unknown flag bit; 8: cap < 0"""
    if T is None:
        return 1
    T = np.asarray(T, dtype=np.float64).reshape(12)
    if not np.isfinite(T).all():
        return 2
    R = T[:9].reshape(3, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            for b in range(3):
                s = (R[a, 0] * R[b, 0] + R[a, 1] * R[b, 1]) + R[a, 2] * R[b, 2]
                if not abs(s - (1.0 if a == b else 0.0)) <= RIGID_TOL:
                    return 3
    if (key_lo is None) != (key_dims is None):
        return 4
    if key_lo is not None:
        if any(int(d) < 1 for d in key_dims):
            return 5
        if any(int(l) + int(d) > I32_MAX for l, d in zip(key_lo, key_dims)):
            return 6
    if flags & ~(SEEN | REPLACE | DRY):
        return 7
    if cap < 0:
        return 8
    return 0


def rot(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0):
    """Rz(yaw) Ry(pitch) Rx(roll), float64"""
    y, p, r = (np.deg2rad(np.float64(v)) for v in (yaw_deg, pitch_deg, roll_deg))
    Rz = np.array([[np.cos(y), -np.sin(y), 0.0], [np.sin(y), np.cos(y), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(p), 0.0, np.sin(p)], [0.0, 1.0, 0.0], [-np.sin(p), 0.0, np.cos(p)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(r), -np.sin(r)], [0.0, np.sin(r), np.cos(r)]])
    return Rz @ Ry @ Rx


def make_T(R=None, o=(0.0, 0.0, 0.0)):
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    return np.concatenate([R.reshape(9), np.asarray(o, dtype=np.float64).reshape(3)])


def invert(T):
    T = np.asarray(T, dtype=np.float64).reshape(12)
    Rt = T[:9].reshape(3, 3).T
    return np.concatenate([Rt.reshape(9), -(Rt @ T[9:])])


def cell_coords(n):
    """(n^3, 3) cell coordinates in cell-index order, x fastest"""
    i = np.arange(n ** 3)
    return np.stack([i % n, (i // n) % n, i // (n * n)], axis=1)


def source_voxels(T, g, n, d_sub):
    """destination blocks g (m, 3) -> (valid (m, C), source voxel (m, C, 3) int64) by the contract's arithmetic"""
    T = np.asarray(T, dtype=np.float64).reshape(12)
    d_sub = np.float64(d_sub)
    d_glb, half = d_sub * np.float64(n), d_sub * np.float64(0.5)
    g = np.asarray(g, dtype=np.int64).reshape(-1, 3).astype(np.float64)
    c = cell_coords(n).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (g[:, None, :] * d_glb + c[None, :, :] * d_sub) + half
        w = np.stack([((T[3 * a] * p[..., 0] + T[3 * a + 1] * p[..., 1]) + T[3 * a + 2] * p[..., 2]) + T[9 + a] for a in range(3)], axis=-1)
        q = np.floor((w / d_sub) * np.float64(1024.0))
        ok = np.abs(q) < np.float64(2.0 ** 40)  # (NaN fails)
    valid = ok.all(axis=-1)
    v = np.where(ok, q, 0.0).astype(np.int64) // 1024
    return valid, v


def candidate_keys(keys, T, n, d_sub, key_lo=None, key_dims=None, margin=2):
    """sorted (m, 3) int64: the destination keys to look at"""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    if not len(keys):
        return np.zeros((0, 3), dtype=np.int64)
    Ti = invert(T)
    Ri, oi = Ti[:9].reshape(3, 3), Ti[9:]
    d_glb = np.float64(d_sub) * n
    corner = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)], dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        img = ((keys[:, None, :] + corner[None, :, :]).astype(np.float64) * d_glb) @ Ri.T + oi
        lo_f, hi_f = np.floor(img.min(axis=1) / d_glb) - margin, np.floor(img.max(axis=1) / d_glb) + margin
    box_lo = np.full(3, KEY_MIN, dtype=np.int64)
    box_hi = np.full(3, KEY_MAX, dtype=np.int64)
    if key_lo is not None:
        box_lo = np.maximum(box_lo, np.asarray(key_lo, dtype=np.int64))
        box_hi = np.minimum(box_hi, np.asarray(key_lo, dtype=np.int64) + np.asarray(key_dims, dtype=np.int64) - 1)
    fine = np.isfinite(lo_f).all(axis=1) & np.isfinite(hi_f).all(axis=1)
    found = set()
    for l, h_ in zip(lo_f[fine], hi_f[fine]):
        l = np.maximum(np.clip(l, -2.0 ** 40, 2.0 ** 40).astype(np.int64), box_lo)
        h_ = np.minimum(np.clip(h_, -2.0 ** 40, 2.0 ** 40).astype(np.int64), box_hi)
        if (l > h_).any():
            continue
        xs, ys, zs = (np.arange(l[a], h_[a] + 1) for a in range(3))
        for x in xs:
            for y in ys:
                found.update((int(x), int(y), int(z)) for z in zs)
    return np.array(sorted(found), dtype=np.int64).reshape(-1, 3)


def warp(blocks, T, n, d_sub, key_lo=None, key_dims=None, seen=False):
    """blocks: {"keys", "log_odds", "occ", "infl"[, "collapsed"]} in any order -> the emitted blocks {"keys" int32, "log_odds" float32,
    "occ", "infl" uint8} in ascending key order and "summary" (int64 [8]; [1], the implementation's candidate count, is -1 here;
    [3] = [2]: everything written)"""
    keys = np.asarray(blocks["keys"], dtype=np.int64).reshape(-1, 3)
    nb, C = len(keys), n ** 3
    lo_s = np.asarray(blocks["log_odds"], dtype=np.float32).reshape(nb, C)
    occ_s = np.asarray(blocks["occ"], dtype=np.uint8).reshape(nb, C)
    infl_s = np.asarray(blocks["infl"], dtype=np.uint8).reshape(nb, C)
    col = np.asarray(blocks.get("collapsed", np.zeros(nb, np.uint8)), dtype=np.uint8).reshape(nb).astype(bool)
    table = {tuple(int(v) for v in k): i for i, k in enumerate(keys)}  # the source blocks
    cand = candidate_keys(keys, T, n, d_sub, key_lo, key_dims)
    out = {"keys": [], "log_odds": [], "occ": [], "infl": []}
    live_n = occ_o = occ_f = infl_o = 0
    chunk = max(1, (1 << 20) // C)  # (destination blocks gathered at a time: a million voxels)
    for c0 in range(0, len(cand), chunk):
        g = cand[c0:c0 + chunk]
        valid, v = source_voxels(T, g, n, d_sub)
        sg = v // n
        sc = v - sg * n
        cell = (sc[..., 2] * n + sc[..., 1]) * n + sc[..., 0]
        in_range = ((sg >= KEY_MIN) & (sg <= KEY_MAX)).all(axis=-1) & valid
        packed = ((sg[..., 0] + (1 << 20)) << 42) | ((sg[..., 1] + (1 << 20)) << 21) | (sg[..., 2] + (1 << 20))
        packed = np.where(in_range, packed, -1)
        uniq, inv = np.unique(packed, return_inverse=True)
        slot_of = np.array([-1 if u < 0 else table.get((int(u >> 42) - (1 << 20), int((u >> 21) & 0x1FFFFF) - (1 << 20), int(u & 0x1FFFFF) - (1 << 20)), -1)
                            for u in uniq], dtype=np.int64)
        slot = slot_of[inv.reshape(packed.shape)]
        present = slot >= 0
        s = np.where(present, slot, 0)
        released = col[s] & present
        cell = np.where(released | ~present, 0, cell)
        L = lo_s[s, cell] if nb else np.zeros(s.shape, np.float32)
        o = occ_s[s, cell] if nb else np.full(s.shape, U, np.uint8)
        i = np.where(released, np.uint8(U), infl_s[s, cell]) if nb else np.full(s.shape, U, np.uint8)
        live = present.copy()
        if seen:
            live &= (o != U) | (i == O)
        L = np.where(live, L, np.float32(0.0)).astype(np.float32)
        o = np.where(live, o, np.uint8(U)).astype(np.uint8)
        i = np.where(live, i, np.uint8(U)).astype(np.uint8)
        emit = live.any(axis=1)
        out["keys"].append(g[emit].astype(np.int32))
        out["log_odds"].append(L[emit])
        out["occ"].append(o[emit])
        out["infl"].append(i[emit])
        live_n += int(live.sum())
        occ_o += int((live & (o == O)).sum())
        occ_f += int((live & (o == F)).sum())
        infl_o += int((live & (i == O)).sum())
    res = {"keys": np.concatenate(out["keys"]).reshape(-1, 3) if out["keys"] else np.zeros((0, 3), np.int32),
           "log_odds": np.concatenate(out["log_odds"]).reshape(-1, C) if out["log_odds"] else np.zeros((0, C), np.float32),
           "occ": np.concatenate(out["occ"]).reshape(-1, C) if out["occ"] else np.zeros((0, C), np.uint8),
           "infl": np.concatenate(out["infl"]).reshape(-1, C) if out["infl"] else np.zeros((0, C), np.uint8)}
    E = len(res["keys"])
    res["summary"] = np.array([nb, -1, E, E, live_n, occ_o, occ_f, infl_o], dtype=np.int64)
    return res


def sorted_blocks(blocks):
    """the blocks in ascending key order (x, then y, then z), released blocks expanded from element 0 with infl 'u'"""
    keys = np.asarray(blocks["keys"], dtype=np.int32).reshape(-1, 3)
    o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    lo, occ, infl = (np.array(np.asarray(blocks[k])[o]) for k in ("log_odds", "occ", "infl"))
    col = np.asarray(blocks.get("collapsed", np.zeros(len(keys), np.uint8)))[o].astype(bool)
    lo[col] = lo[col][:, :1]
    occ[col] = occ[col][:, :1]
    infl[col] = U
    return {"keys": keys[o], "log_odds": lo, "occ": occ, "infl": infl}
