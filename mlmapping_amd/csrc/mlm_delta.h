// mlm_delta.h — the rule of mlm_delta_blocks (include/mlmap_hip.h): the argument check with its codes and texts, the view of a block,
// the word of a voxel and the mixer the digest sums, the three-way classification of the join and the order of the tables — once, for
// the kernels (mlm_kernels_delta.h), the host driver (mlm_delta_host.h) and the CPU test driver (tests/cpp/delta_driver.cpp), so that
// all three run the very same arithmetic.  No reference counterpart: the reference hands its whole map out every time.
//
// The view of a block: its `cells` triples (log-odds bits, occ, infl) as mlm_warp_blocks reads them — a released block of a
// frontier-mode handle answers from element 0 with infl 'u' in every cell — and with MLM_DELTA_NO_INFL infl is 'u' everywhere.  The
// emitted planes are the view.
//
// The digest of a block: two uint64 in arithmetic mod 2^64 over the cell index c = 0 .. cells - 1 of the view,
//     w_c  = bits(L_c) | (uint64)occ_c << 32 | (uint64)infl_c << 40
//     x_c  = w_c ^ ((c + 1) * 0x9E3779B97F4A7C15)
//     f(x) : x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
//     d[0] = sum_c f(x_c)          d[1] = sum_c f(x_c ^ 0xD6E8FEB86659FD93)
// A sum of integers: one value whatever the schedule, no atomic and no float.  Over the bits: -0.0f and +0.0f differ.
//
// The join.  A block of the map is SELECTED iff its key lies inside the key box (no box: every block).  A selected block is UNCHANGED
// (its key is in the previous table with an equal digest), CHANGED (in it with another digest) or NEW (not in it); a row of the
// previous table inside the box whose key the map does not hold is GONE; rows outside the box are ignored.  Tables, emitted blocks and
// gone keys are ordered by the packed key (mlm_warp_pack): x, then y, then z, ascending.
#pragma once
#include <stdint.h>

#include "mlm_age.h"
#include "mlm_warp.h"

// (the values of include/mlmap_hip.h; mlm_delta_host.h holds them to each other)
#define MLM_DELTA_F_DRY 1
#define MLM_DELTA_F_NO_INFL 2
#define MLM_DELTA_F_ALL 3
#define MLM_DELTA_SUMS 12 // int64 of the summary

#define MLM_DELTA_K_UNCHANGED 0
#define MLM_DELTA_K_CHANGED 1 // (the values of the `kind` output)
#define MLM_DELTA_K_NEW 2
#define MLM_DELTA_K_NONE 3 // (scratch only: a slot the call did not select)

// a row of the previous table
#define MLM_DELTA_P_OUTSIDE 0
#define MLM_DELTA_P_HELD 1
#define MLM_DELTA_P_GONE 2

#define MLM_DELTA_GOLD 0x9E3779B97F4A7C15ull
#define MLM_DELTA_SECOND 0xD6E8FEB86659FD93ull

// 0: fine (S is filled); 1: one of key_lo / key_dims null and the other not; 2: a key dim < 1; 3: key_lo + key_dims beyond int32
// (mlm_crop_check's 2 and 3, with its texts); 4: an unknown flag bit; 5: a negative cap or n_prev; 6: n_prev > 0 with a null table;
// 7: a previous key outside the 21-bit range; 8: previous keys not strictly ascending (7 and 8 are found where the table is read)
MLM_CROP_HD int mlm_delta_check(const int32_t *key_lo, const int32_t *key_dims, long long n_prev, const void *prev_keys, const void *prev_digest, int flags,
                                long long cap_table, long long cap, long long cap_gone, MlmAgeSel &S) {
    if ((key_lo == nullptr) != (key_dims == nullptr)) return 1;
    S.all = key_lo ? 0 : 1;
    if (key_lo) {
        const int bad = mlm_crop_check(key_lo, key_dims, 0, 0, S.B);
        if (bad) return bad; // (2 or 3: the box is given, no flag, cap 0)
    } else {
        for (int a = 0; a < 3; ++a) S.B.lo[a] = S.B.hi[a] = 0;
    }
    S.B.inside = 1;
    if (flags & ~MLM_DELTA_F_ALL) return 4;
    if (cap_table < 0 || cap < 0 || cap_gone < 0 || n_prev < 0) return 5;
    if (n_prev > 0 && (!prev_keys || !prev_digest)) return 6;
    return 0;
}
MLM_CROP_HD const char *mlm_delta_check_text(int bad) {
    return bad == 1   ? "key_lo and key_dims must be given together"
           : bad <= 4 ? mlm_crop_check_text(bad)
           : bad == 5 ? "cap_table, cap, cap_gone and n_prev must be >= 0"
           : bad == 6 ? "n_prev > 0 takes prev_keys and prev_digest"
           : bad == 7 ? "a previous key lies outside the 21-bit key range"
                      : "the previous keys must be strictly ascending by packed key";
}

// the order: the packed key of a row of a key table
MLM_CROP_HD unsigned long long mlm_delta_pack3(const int32_t *k) {
    const int g[3] = {k[0], k[1], k[2]};
    return mlm_warp_pack(g);
}
MLM_CROP_HD bool mlm_delta_key_ok(const int32_t *k) {
    const int g[3] = {k[0], k[1], k[2]};
    return mlm_warp_key_ok(g);
}

// the voxel's word, the mixer, and what cell c adds to the digest (cg = (c + 1) * MLM_DELTA_GOLD)
MLM_CROP_HD unsigned long long mlm_delta_word(uint32_t lo_bits, uint8_t occ, uint8_t infl) {
    return (unsigned long long)lo_bits | (unsigned long long)occ << 32 | (unsigned long long)infl << 40;
}
MLM_CROP_HD unsigned long long mlm_delta_mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
MLM_CROP_HD void mlm_delta_cell(unsigned long long cg, unsigned long long w, unsigned long long &d0, unsigned long long &d1) {
    const unsigned long long x = w ^ cg;
    d0 += mlm_delta_mix(x);
    d1 += mlm_delta_mix(x ^ MLM_DELTA_SECOND);
}

// the three-way classification of a selected block
MLM_CROP_HD int mlm_delta_kind(bool in_prev, bool same_digest) { return !in_prev ? MLM_DELTA_K_NEW : same_digest ? MLM_DELTA_K_UNCHANGED : MLM_DELTA_K_CHANGED; }
MLM_CROP_HD bool mlm_delta_emits(int kind) { return kind == MLM_DELTA_K_CHANGED || kind == MLM_DELTA_K_NEW; }

// first index i of the n ascending packed keys at(i) with at(i) >= key (n: none)
template <class At> MLM_CROP_HD uint32_t mlm_delta_lower_bound(At at, uint32_t n, unsigned long long key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (at(mid) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
