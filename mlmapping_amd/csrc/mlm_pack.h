// mlm_pack.h — the rule of mlm_pack_blocks / mlm_unpack_blocks (include/mlmap_hip.h): the argument checks with their codes and texts,
// the code of a cell, the size of a record from (presence, n_lit), the header and the validator of a stream — once, for the kernels
// (mlm_kernels_pack.h), the host driver (mlm_pack_host.h) and the CPU test driver (tests/cpp/pack_driver.cpp), so that all three run
// the very same arithmetic.  No reference counterpart: the reference hands its map out voxel by voxel.
//
// The stream, little endian.  C = subbox_n^3 cells per block, W = ceil(C / 64); a PLANE is W uint64, bit i of word j belongs to cell
// 64 j + i, bits of cells >= C are zero.
//     header, 64 bytes: "MLMPACK1" | u32 C | u32 subbox_n | u32 n | u32 flags (bit 0: infl left out) | u32 bits of lo_min | u32 bits of
//                       lo_max | u64 total bytes | u64 literals | 16 zero bytes
//     directory, 16 bytes per block in row order: int32 key[3] | u32 offset of the record in 8-byte units from the start of the stream
//     records, back to back in row order, each 8-byte aligned: u32 presence (bits 0..5) | u32 n_lit | the present planes in the order
//                       occ0 occ1 infl0 infl1 val0 val1 | n_lit uint32 literals | zero padding to 8 bytes
// The code of a cell: occ and infl 'u' 0, 'f' 1, 'o' 2 (bit 0 in plane 0, bit 1 in plane 1); val, on the log-odds BITS in this order: 0
// zero, 1 the header's lo_min bits, 2 its lo_max bits, 3 anything else — and such a cell appends its 32 bits to the literals, in cell
// order.  The encoder writes a plane iff it has a set bit: one byte string per input.
//
// The validator.  Block i is judged on its own from its directory row: its offset o_i, the two words at 8 o_i, its planes; and it
// judges the offset of its successor (o_{i+1} must be o_i + its size; the last record must end at the total).  The verdict of a stream
// is the failure with the smallest (block, check number); every read is preceded by a comparison against `total`, and total <= bytes.
#pragma once
#include <stdint.h>

#include "mlm_delta.h"

// (the values of include/mlmap_hip.h; mlm_pack_host.h holds them to each other)
#define MLM_PACK_F_DRY 1
#define MLM_PACK_F_NO_INFL 2
#define MLM_PACK_F_ALL 3
#define MLM_PACK_SUMS 8 // int64 of the summary
#define MLM_PACK_HEADER 64
#define MLM_PACK_DIR 16
#define MLM_PACK_MAX_UNITS 0xFFFFFFFFull // a stream holds at most 2^32 - 1 eight-byte units: the directory's offsets are u32

// what pass 1 / the validator leave per row: the record's size in 8-byte units, its literals, its cells coded lo_min and lo_max, its
// presence bits; err: 0, or what is wrong with the row (pack: 1 a byte outside 'u' 'f' 'o'; unpack: the check number)
struct MlmPackRow {
    uint32_t units, n_lit, n_min, n_max, presence, err, pad0, pad1;
};

MLM_CROP_HD uint32_t mlm_pack_words(uint32_t C) { return (C + 63u) / 64u; }
// bytes of a record (a multiple of 8)
MLM_CROP_HD unsigned long long mlm_pack_record_bytes(uint32_t W, uint32_t presence, uint32_t n_lit) {
    return 8ull + 8ull * W * (unsigned long long)__builtin_popcount(presence & 63u) + ((4ull * n_lit + 7ull) & ~7ull);
}
// bytes of the header and the directory of n blocks; raw bytes of n blocks of a dump
MLM_CROP_HD unsigned long long mlm_pack_front_bytes(unsigned long long n) { return MLM_PACK_HEADER + MLM_PACK_DIR * n; }
MLM_CROP_HD unsigned long long mlm_pack_raw_bytes(unsigned long long n, uint32_t C) { return n * (12ull + 6ull * C); }

// the code of an occ / infl byte (3: not one of 'u' 'f' 'o') and its inverse
MLM_CROP_HD uint32_t mlm_pack_class_code(uint8_t b) { return b == (uint8_t)'u' ? 0u : b == (uint8_t)'f' ? 1u : b == (uint8_t)'o' ? 2u : 3u; }
MLM_CROP_HD uint8_t mlm_pack_class_byte(uint32_t code) { return code == 0u ? (uint8_t)'u' : code == 1u ? (uint8_t)'f' : (uint8_t)'o'; }
// the code of a log-odds word, decided on its bits in this order
MLM_CROP_HD uint32_t mlm_pack_val_code(uint32_t bits, uint32_t min_bits, uint32_t max_bits) { return bits == 0u ? 0u : bits == min_bits ? 1u : bits == max_bits ? 2u : 3u; }
MLM_CROP_HD uint32_t mlm_pack_val_bits(uint32_t code, uint32_t min_bits, uint32_t max_bits, uint32_t literal) {
    return code == 0u ? 0u : code == 1u ? min_bits : code == 2u ? max_bits : literal;
}
// bits of word j of a plane that belong to no cell
MLM_CROP_HD unsigned long long mlm_pack_tail_mask(uint32_t C, uint32_t j) {
    const uint32_t first = 64u * j;
    return first + 64u <= C ? 0ull : first >= C ? ~0ull : ~0ull << (C - first);
}

// mlm_pack_blocks' arguments.  0: fine (S is filled); 1: one of key_lo / key_dims null and the other not; 2: a key dim < 1; 3: key_lo +
// key_dims beyond int32 (mlm_crop_check's, with its texts); 4: an unknown flag bit; 5: a key box together with rows; 6: a negative n;
// 7: rows without log_odds or occ; 8: a device stream that is not 8-byte aligned; 9: an occ or infl byte outside 'u' 'f' 'o' (found on
// the device)
MLM_CROP_HD int mlm_pack_check(const int32_t *key_lo, const int32_t *key_dims, long long n, const void *keys, const void *log_odds, const void *occ, int flags,
                               bool device_stream, unsigned long long stream_addr, MlmAgeSel &S) {
    if ((key_lo == nullptr) != (key_dims == nullptr)) return 1;
    S.all = key_lo ? 0 : 1;
    if (key_lo) {
        const int bad = mlm_crop_check(key_lo, key_dims, 0, 0, S.B);
        if (bad) return bad; // (2 or 3: the box is given, no flag, cap 0)
    } else {
        for (int a = 0; a < 3; ++a) S.B.lo[a] = S.B.hi[a] = 0;
    }
    S.B.inside = 1;
    if (flags & ~MLM_PACK_F_ALL) return 4;
    if (keys && key_lo) return 5;
    if (n < 0) return 6;
    if (keys && n > 0 && (!log_odds || !occ)) return 7;
    if (device_stream && (stream_addr & 7ull)) return 8;
    return 0;
}
MLM_CROP_HD const char *mlm_pack_check_text(int bad) {
    return bad == 1   ? "key_lo and key_dims must be given together"
           : bad <= 4 ? mlm_crop_check_text(bad)
           : bad == 5 ? "a key box selects blocks of the live map: it does not go with rows"
           : bad == 6 ? "n must be >= 0"
           : bad == 7 ? "rows take keys, log_odds and occ"
           : bad == 8 ? "a stream in device memory must be 8-byte aligned"
                      : "an occ or infl byte is none of 'u' 'f' 'o'";
}

// mlm_unpack_blocks' checks, by number.  Of the arguments: 11 a null stream; 12 an unknown flag bit; 13 a negative cap; 14 a device
// stream that is not 8-byte aligned.  Of the stream: 1 bytes below the header; 2 a wrong magic; 3 C or subbox_n not the handle's; 4 the
// header's total above bytes or below header + directory; 5 a directory offset that is not the previous record's end; 6 presence >= 64;
// 7 a set bit for a cell >= C; 8 an occ or infl code 3; 9 n_lit other than the popcount of val0 & val1; 10 a record running past the
// total, or the last one ending short of it
MLM_CROP_HD const char *mlm_unpack_check_text(int bad) {
    return bad == 1    ? "check 1: fewer bytes than the header"
           : bad == 2  ? "check 2: the magic is not MLMPACK1"
           : bad == 3  ? "check 3: C or subbox_n is not this handle's"
           : bad == 4  ? "check 4: the header's total does not lie between header + directory and bytes"
           : bad == 5  ? "check 5: a directory offset is not the previous record's end"
           : bad == 6  ? "check 6: presence >= 64"
           : bad == 7  ? "check 7: a bit is set for a cell >= C"
           : bad == 8  ? "check 8: an occ or infl code 3"
           : bad == 9  ? "check 9: n_lit is not the popcount of val0 & val1"
           : bad == 10 ? "check 10: a record does not end within the total"
           : bad == 11 ? "check 11: null stream"
           : bad == 12 ? "check 12: unknown flag bit"
           : bad == 13 ? "check 13: cap must be >= 0"
                       : "check 14: a stream in device memory must be 8-byte aligned";
}
MLM_CROP_HD int mlm_unpack_check(const void *stream, int flags, long long cap, bool device_stream, unsigned long long stream_addr) {
    if (!stream) return 11;
    if (flags) return 12;
    if (cap < 0) return 13;
    if (device_stream && (stream_addr & 7ull)) return 14;
    return 0;
}

// little-endian words of the stream: byte by byte on the host (any alignment), one load on the device (the stream is 8-byte aligned
// there, every u32 of the format lies at a multiple of 4 and every u64 at a multiple of 8)
MLM_CROP_HD uint32_t mlm_pack_u32(const uint8_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *(const uint32_t *)p;
#else
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
#endif
}
MLM_CROP_HD unsigned long long mlm_pack_u64(const uint8_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *(const unsigned long long *)p;
#else
    return (unsigned long long)mlm_pack_u32(p) | (unsigned long long)mlm_pack_u32(p + 4) << 32;
#endif
}
MLM_CROP_HD void mlm_pack_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24); }

struct MlmPackHeader {
    uint32_t C, subbox_n, n, flags, min_bits, max_bits;
    unsigned long long total, literals;
};
// the 64 bytes of a header
MLM_CROP_HD void mlm_pack_header_write(const MlmPackHeader &H, uint8_t out[MLM_PACK_HEADER]) {
    const char magic[9] = "MLMPACK1";
    for (int i = 0; i < 8; ++i) out[i] = (uint8_t)magic[i];
    mlm_pack_put32(out + 8, H.C), mlm_pack_put32(out + 12, H.subbox_n), mlm_pack_put32(out + 16, H.n), mlm_pack_put32(out + 20, H.flags);
    mlm_pack_put32(out + 24, H.min_bits), mlm_pack_put32(out + 28, H.max_bits);
    mlm_pack_put32(out + 32, (uint32_t)H.total), mlm_pack_put32(out + 36, (uint32_t)(H.total >> 32));
    mlm_pack_put32(out + 40, (uint32_t)H.literals), mlm_pack_put32(out + 44, (uint32_t)(H.literals >> 32));
    for (int i = 48; i < MLM_PACK_HEADER; ++i) out[i] = 0;
}
// checks 1 .. 4: `have` bytes of the stream are at `head` (64 of them are read, and only if bytes >= 64)
MLM_CROP_HD int mlm_pack_header_check(const uint8_t *head, unsigned long long bytes, uint32_t C, uint32_t subbox_n, MlmPackHeader &H) {
    if (bytes < MLM_PACK_HEADER) return 1;
    const char magic[9] = "MLMPACK1";
    for (int i = 0; i < 8; ++i)
        if (head[i] != (uint8_t)magic[i]) return 2;
    H.C = mlm_pack_u32(head + 8), H.subbox_n = mlm_pack_u32(head + 12), H.n = mlm_pack_u32(head + 16), H.flags = mlm_pack_u32(head + 20);
    H.min_bits = mlm_pack_u32(head + 24), H.max_bits = mlm_pack_u32(head + 28);
    H.total = mlm_pack_u64(head + 32), H.literals = mlm_pack_u64(head + 40);
    if (H.C != C || H.subbox_n != subbox_n) return 3;
    if (H.total > bytes || H.total < mlm_pack_front_bytes(H.n)) return 4;
    return 0;
}

// The validator of block i < n, in three steps.  `s` is the stream, of which [0, total) may be read; total >= header + directory.
// open: the directory row and the record's two leading words -> o (offset in units), presence, n_lit, size (bytes); 0, 5 (block 0 only:
// its offset is not the directory's end), 6 or 10.  The planes may be read after a 0 only.
MLM_CROP_HD int mlm_pack_block_open(const uint8_t *s, unsigned long long total, uint32_t W, uint32_t n, uint32_t i, unsigned long long &o, uint32_t &presence, uint32_t &n_lit,
                                    unsigned long long &size) {
    o = mlm_pack_u32(s + MLM_PACK_HEADER + MLM_PACK_DIR * (unsigned long long)i + 12);
    presence = n_lit = 0, size = 0;
    if (i == 0 && 8ull * o != mlm_pack_front_bytes(n)) return 5; // (the smallest (block, check) there is: nothing else is looked at)
    if (8ull * o + 8ull > total) return 10;
    presence = mlm_pack_u32(s + 8ull * o), n_lit = mlm_pack_u32(s + 8ull * o + 4);
    if (presence >= 64u) return 6;
    size = mlm_pack_record_bytes(W, presence, n_lit);
    if (8ull * o + size > total) return 10;
    return 0;
}
// word j of the six planes of an opened record (absent planes are zero)
MLM_CROP_HD void mlm_pack_block_words(const uint8_t *s, unsigned long long o, uint32_t W, uint32_t presence, uint32_t j, unsigned long long w[6]) {
    const uint8_t *p = s + 8ull * o + 8ull;
    for (int k = 0; k < 6; ++k) {
        w[k] = 0ull;
        if (presence >> k & 1u) {
            w[k] = mlm_pack_u64(p + 8ull * j);
            p += 8ull * W;
        }
    }
}
// what word j adds: flag bit 0 a tail bit (check 7), bit 1 a code 3 (check 8); the literals and the cells coded lo_min / lo_max
MLM_CROP_HD uint32_t mlm_pack_word_check(const unsigned long long w[6], uint32_t C, uint32_t j, uint32_t &n_lit, uint32_t &n_min, uint32_t &n_max) {
    const unsigned long long tail = mlm_pack_tail_mask(C, j);
    uint32_t f = 0;
    if ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5]) & tail) f |= 1u;
    if ((w[0] & w[1]) | (w[2] & w[3])) f |= 2u;
    n_lit += (uint32_t)__builtin_popcountll(w[4] & w[5]);
    n_min += (uint32_t)__builtin_popcountll(w[4] & ~w[5]);
    n_max += (uint32_t)__builtin_popcountll(~w[4] & w[5]);
    return f;
}
// close: the verdict of the block from open's code, the flags of its words and its literal count; next: 5 if the successor's offset is
// not this record's end (block i + 1 fails check 5), else 0.  A record that was not opened judges no successor.
MLM_CROP_HD int mlm_pack_block_close(const uint8_t *s, unsigned long long total, uint32_t n, uint32_t i, int opened, unsigned long long o, unsigned long long size, uint32_t flags,
                                     uint32_t n_lit_header, uint32_t n_lit_planes, int &next) {
    next = 0;
    if (opened) return opened;
    const unsigned long long end = 8ull * o + size;
    bool short_of_total = false;
    if (i + 1u < n) next = mlm_pack_u32(s + MLM_PACK_HEADER + MLM_PACK_DIR * (unsigned long long)(i + 1u) + 12) * 8ull != end ? 5 : 0;
    else short_of_total = end != total;
    if (flags & 1u) return 7;
    if (flags & 2u) return 8;
    if (n_lit_header != n_lit_planes) return 9;
    return short_of_total ? 10 : 0;
}
// the verdict of a stream from its rows: the smallest (block, check); `next_err` of block i - 1 counts for block i
MLM_CROP_HD unsigned long long mlm_pack_verdict_key(uint32_t i, uint32_t own, uint32_t from_prev) {
    const uint32_t code = from_prev && (own == 0 || from_prev < own) ? from_prev : own;
    return code ? (unsigned long long)i << 8 | code : ~0ull;
}
