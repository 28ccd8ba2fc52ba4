"""The contract of mlm_pack_blocks / mlm_unpack_blocks (include/mlmap_hip.h) in numpy: planes by np.packbits(..., bitorder="little"),
the canonical encoder, and the validating decoder with the header's check numbers.  Written from the header's text, apart from
mlmapping_amd/csrc/mlm_pack.h: the encoder builds whole planes per block instead of words per step, the decoder collects every failure
of every block in a list and takes the smallest (block, check)."""
import struct

import numpy as np

from tests import delta_ref

DRY, NO_INFL, ALL_FLAGS = 1, 2, 3
ROW = 8
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3
U, F, O = ord("u"), ord("f"), ord("o")
MAGIC = b"MLMPACK1"
HEADER, DIR = 64, 16
MAX_UNITS = (1 << 32) - 1
PACK_TEXTS = {1: "key_lo and key_dims must be given together", 2: "key_dims must be >= 1", 3: "key_lo + key_dims must fit an int32", 4: "unknown flag bit",
              5: "a key box selects blocks of the live map: it does not go with rows", 6: "n must be >= 0", 7: "rows take keys, log_odds and occ",
              8: "a stream in device memory must be 8-byte aligned", 9: "an occ or infl byte is none of 'u' 'f' 'o'"}
UNPACK_TEXTS = {1: "check 1: fewer bytes than the header", 2: "check 2: the magic is not MLMPACK1", 3: "check 3: C or subbox_n is not this handle's",
                4: "check 4: the header's total does not lie between header + directory and bytes", 5: "check 5: a directory offset is not the previous record's end",
                6: "check 6: presence >= 64", 7: "check 7: a bit is set for a cell >= C", 8: "check 8: an occ or infl code 3",
                9: "check 9: n_lit is not the popcount of val0 & val1", 10: "check 10: a record does not end within the total", 11: "check 11: null stream",
                12: "check 12: unknown flag bit", 13: "check 13: cap must be >= 0", 14: "check 14: a stream in device memory must be 8-byte aligned"}


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def words(C):
    return (C + 63) // 64


def record_bytes(W, presence, n_lit):
    return 8 + 8 * W * bin(presence & 63).count("1") + (4 * n_lit + 7) // 8 * 8


def plane(bits, W):
    """W little-endian uint64 of the 0/1 array bits [C] as bytes"""
    padded = np.zeros(64 * W, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").tobytes()


def class_codes(a):
    a = np.asarray(a, dtype=np.uint8)
    code = np.full(a.shape, 3, dtype=np.uint8)
    code[a == U], code[a == F], code[a == O] = 0, 1, 2
    return code


def val_codes(bits, min_bits, max_bits):
    """decided in this order: zero, lo_min, lo_max, literal"""
    code = np.full(bits.shape, 3, dtype=np.uint8)
    code[bits == max_bits] = 2
    code[bits == min_bits] = 1
    code[bits == 0] = 0
    return code


def record(lo_bits, occ, infl, min_bits, max_bits):
    """the canonical record of one block (bytes), and (n_lit, n_min, n_max)"""
    C = len(lo_bits)
    W = words(C)
    co, ci, cv = class_codes(occ), class_codes(infl), val_codes(lo_bits, min_bits, max_bits)
    six = [co & 1, co >> 1, ci & 1, ci >> 1, cv & 1, cv >> 1]
    presence = sum(1 << k for k, p in enumerate(six) if p.any())
    lits = np.ascontiguousarray(lo_bits[cv == 3], dtype="<u4")
    body = b"".join(plane(p, W) for k, p in enumerate(six) if presence >> k & 1) + lits.tobytes()
    out = struct.pack("<II", presence, len(lits)) + body + b"\0" * (-len(body) % 8)
    assert len(out) == record_bytes(W, presence, len(lits))
    return out, (len(lits), int((cv == 1).sum()), int((cv == 2).sum()))


def pack_rows(keys, log_odds, occ, infl, subbox_n, lo_min, lo_max, no_infl=False):
    """n rows of a dump in row order -> {"status", "code", "row"} or {"status", "stream": bytes, "summary": int64 [8]} ([7] as a call that
    writes reports it)"""
    C = subbox_n ** 3
    keys = np.asarray(keys, dtype=np.int32).reshape(-1, 3)
    n = len(keys)
    bits = np.ascontiguousarray(log_odds, dtype=np.float32).reshape(n, C).view(np.uint32)
    occ = np.asarray(occ, dtype=np.uint8).reshape(n, C)
    infl = np.full((n, C), U, dtype=np.uint8) if infl is None or no_infl else np.asarray(infl, dtype=np.uint8).reshape(n, C)
    bad = np.nonzero(((class_codes(occ) == 3) | (class_codes(infl) == 3)).any(axis=1))[0]
    if len(bad):
        return {"status": ERR_INVALID, "code": 9, "row": int(bad[0])}
    min_bits, max_bits = f32_bits(lo_min), f32_bits(lo_max)
    recs, counts = [], np.zeros(3, dtype=np.int64)
    for r in range(n):
        rec, c = record(bits[r], occ[r], infl[r], min_bits, max_bits)
        recs.append(rec)
        counts += c
    front = HEADER + DIR * n
    total = front + sum(len(r) for r in recs)
    summary = np.array([n, total, n * (12 + 6 * C), sum(len(r) == 8 for r in recs), counts[0], counts[1], counts[2], total], dtype=np.int64)
    if total // 8 > MAX_UNITS:
        return {"status": ERR_CAPACITY, "summary": summary}
    head = MAGIC + struct.pack("<6I2Q", C, subbox_n, n, 1 if no_infl else 0, min_bits, max_bits, total, int(counts[0])) + b"\0" * 16
    directory, at = [], front
    for k, rec in zip(keys, recs):
        directory.append(struct.pack("<3iI", int(k[0]), int(k[1]), int(k[2]), at // 8))
        at += len(rec)
    stream = head + b"".join(directory) + b"".join(recs)
    assert len(stream) == total and len(head) == HEADER
    return {"status": OK, "code": 0, "stream": stream, "summary": summary}


def pack_map(b, subbox_n, lo_min, lo_max, key_lo=None, key_dims=None, no_infl=False):
    """the live-map source: the blocks of the key box, ascending by packed key, through mlm_delta_blocks' view"""
    keys = np.asarray(b["keys"], dtype=np.int32).reshape(-1, 3)
    lo, occ, infl = delta_ref.view(b, no_infl)
    sel = np.nonzero(delta_ref.in_box(keys, key_lo, key_dims))[0]
    sel = sel[delta_ref.order(keys[sel])]
    return pack_rows(keys[sel], lo[sel], occ[sel], infl[sel], subbox_n, lo_min, lo_max, no_infl)


def verdict(buf, C, subbox_n):
    """(check number or 0, block or -1, header fields or None) of any byte string"""
    if len(buf) < HEADER:
        return 1, -1, None
    if buf[:8] != MAGIC:
        return 2, -1, None
    hC, hn_sub, n, flags, min_bits, max_bits, total, lits = struct.unpack_from("<6I2Q", buf, 8)
    if (hC, hn_sub) != (C, subbox_n):
        return 3, -1, None
    if total > len(buf) or total < HEADER + DIR * n:
        return 4, -1, None
    W = words(C)
    offs = [struct.unpack_from("<I", buf, HEADER + DIR * i + 12)[0] for i in range(n)]
    fails = []
    tail = np.zeros(64 * W, dtype=bool)
    tail[C:] = True
    for i, o in enumerate(offs):
        if i == 0 and 8 * o != HEADER + DIR * n:
            fails.append((0, 5))
        if 8 * o + 8 > total:
            fails.append((i, 10))
            continue
        presence, n_lit = struct.unpack_from("<II", buf, 8 * o)
        if presence >= 64:
            fails.append((i, 6))
            continue
        end = 8 * o + record_bytes(W, presence, n_lit)
        if end > total:
            fails.append((i, 10))
            continue
        if i + 1 < n:
            if 8 * offs[i + 1] != end:
                fails.append((i + 1, 5))
        elif end != total:
            fails.append((i, 10))
        six = block_planes(buf, o, W, presence)
        if any(p[tail].any() for p in six):
            fails.append((i, 7))
        if (six[0] & six[1]).any() or (six[2] & six[3]).any():
            fails.append((i, 8))
        if int((six[4] & six[5]).sum()) != n_lit:
            fails.append((i, 9))
    if fails:
        blk, code = min(fails)
        return code, blk, None
    return 0, -1, (n, flags, min_bits, max_bits, total, lits, offs)


def block_planes(buf, o, W, presence):
    """the six planes of the record at unit o as bool [64 W] (absent planes zero)"""
    six, at = [], 8 * o + 8
    for k in range(6):
        if presence >> k & 1:
            six.append(np.unpackbits(np.frombuffer(buf, dtype=np.uint8, count=8 * W, offset=at), bitorder="little").astype(bool))
            at += 8 * W
        else:
            six.append(np.zeros(64 * W, dtype=bool))
    return six


def unpack(buf, subbox_n):
    """{"status", "code", "block"} or the rows: "keys", "log_odds", "occ", "infl", "summary" int64 [8] ([7] as a call that writes all four)"""
    buf = bytes(buf)
    C = subbox_n ** 3
    code, blk, hdr = verdict(buf, C, subbox_n)
    if code:
        return {"status": ERR_INVALID, "code": code, "block": blk}
    n, flags, min_bits, max_bits, total, lits, offs = hdr
    W = words(C)
    keys = np.zeros((n, 3), dtype=np.int32)
    bits = np.zeros((n, C), dtype=np.uint32)
    occ, infl = np.zeros((n, C), dtype=np.uint8), np.zeros((n, C), dtype=np.uint8)
    letters = np.array([U, F, O, O], dtype=np.uint8)
    counts = np.zeros(4, dtype=np.int64)
    for i, o in enumerate(offs):
        keys[i] = struct.unpack_from("<3i", buf, HEADER + DIR * i)
        presence, n_lit = struct.unpack_from("<II", buf, 8 * o)
        six = [p[:C].astype(np.uint8) for p in block_planes(buf, o, W, presence)]
        occ[i], infl[i] = letters[six[0] | six[1] << 1], letters[six[2] | six[3] << 1]
        cv = six[4] | six[5] << 1
        bits[i][cv == 1], bits[i][cv == 2] = min_bits, max_bits
        bits[i][cv == 3] = np.frombuffer(buf, dtype="<u4", count=n_lit, offset=8 * o + 8 + 8 * W * bin(presence).count("1"))
        counts += [record_bytes(W, presence, n_lit) == 8, n_lit, (cv == 1).sum(), (cv == 2).sum()]
    summary = np.array([n, total, n * (12 + 6 * C), counts[0], counts[1], counts[2], counts[3], n * (12 + 6 * C)], dtype=np.int64)
    return {"status": OK, "code": 0, "keys": keys, "log_odds": bits.view(np.float32), "occ": occ, "infl": infl, "summary": summary, "no_infl": bool(flags & 1)}
