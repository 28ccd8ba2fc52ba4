// mlm_crop.h — the plan of mlm_crop_blocks (include/mlmap_hip.h): the argument check, the predicate that says which blocks a key box
// drops, the hole-filling rule that compacts the pool in place and the shrink rule, once, for the kernels (mlm_kernels_crop.h), the
// host driver (mlmap_hip.hip) and the CPU test driver (tests/cpp/crop_driver.cpp), so that all three run the very same arithmetic.
// No reference counterpart: the reference's observed_group_map only ever grows (allocate_ram, map_local.h:215-231).
//
// The rule.  nb blocks are in use, slot s is dropped iff drop[s]; d(s) is the exclusive prefix sum of drop, D = d(nb), K = nb - D,
// H = d(K) — the dropped slots below K, which is also the number of kept slots at or above K.
//     a dropped slot s <  K is hole   number d(s);
//     a kept    slot s >= K is filler number s - d(s) - (K - H);
//     filler j moves into hole j;  the dropped block of old slot s is output row d(s).
// Afterwards slots [0, K) are in use and [K, nb) are free.  Sources (>= K) and destinations (< K) are disjoint: the moves have no
// order among them, and the slot order after the call is one answer whatever the schedule.  At most min(D, K) blocks move.
//
// Both kinds of slot are found through ONE list of nb entries, the stable partition of the slots: the dropped ones in ascending order
// in front, the kept ones in ascending order behind them (mlm_crop_list_pos).  Output row r is slot list[r]; hole j is list[j];
// filler j is list[D + (K - H) + j] (the kept slots below K stay where they are).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MLM_CROP_HD __host__ __device__ __forceinline__
#else
#define MLM_CROP_HD inline
#endif

// (the values of include/mlmap_hip.h; mlmap_hip.hip holds them to each other)
#define MLM_CROP_F_INSIDE 1
#define MLM_CROP_F_DRY 2
#define MLM_CROP_F_SHRINK 4
#define MLM_CROP_F_ALL 7
#define MLM_CROP_SLOTS_PER_CHUNK 2048 // slots whose drop flags one workgroup counts and ranks (a multiple of the workgroup)

struct MlmCropBox {
    int32_t lo[3], hi[3]; // first and last block key per axis (inclusive)
    int32_t inside;       // 1: keys inside the box are dropped; 0: keys outside it
};

// 0: fine (B is filled); 1: no box; 2: a dim < 1; 3: key_lo + key_dims beyond int32; 4: an unknown flag bit; 5: cap < 0
MLM_CROP_HD int mlm_crop_check(const int32_t *key_lo, const int32_t *key_dims, int flags, long long cap, MlmCropBox &B) {
    if (!key_lo || !key_dims) return 1;
    for (int a = 0; a < 3; ++a)
        if (key_dims[a] < 1) return 2;
    for (int a = 0; a < 3; ++a)
        if ((long long)key_lo[a] + key_dims[a] > 0x7FFFFFFFll) return 3;
    if (flags & ~MLM_CROP_F_ALL) return 4;
    if (cap < 0) return 5;
    for (int a = 0; a < 3; ++a) {
        B.lo[a] = key_lo[a];
        B.hi[a] = (int32_t)((long long)key_lo[a] + key_dims[a] - 1);
    }
    B.inside = (flags & MLM_CROP_F_INSIDE) ? 1 : 0;
    return 0;
}
MLM_CROP_HD const char *mlm_crop_check_text(int bad) {
    return bad == 1   ? "null key box"
           : bad == 2 ? "key_dims must be >= 1"
           : bad == 3 ? "key_lo + key_dims must fit an int32"
           : bad == 4 ? "unknown flag bit"
                      : "cap must be >= 0";
}

// is the block with this key dropped?
MLM_CROP_HD bool mlm_crop_drops(const MlmCropBox &B, int32_t kx, int32_t ky, int32_t kz) {
    const bool in = kx >= B.lo[0] && kx <= B.hi[0] && ky >= B.lo[1] && ky <= B.hi[1] && kz >= B.lo[2] && kz <= B.hi[2];
    return in == (B.inside != 0);
}

// where slot s stands in the list: d = d(s), D = d(nb)
MLM_CROP_HD uint32_t mlm_crop_list_pos(uint32_t s, uint32_t d, bool dropped, uint32_t D) { return dropped ? d : D + (s - d); }
// the pair j < H of the move: list index of its hole (destination, < K) and of its filler (source, >= K)
MLM_CROP_HD uint32_t mlm_crop_hole_at(uint32_t j) { return j; }
MLM_CROP_HD uint32_t mlm_crop_filler_at(uint32_t j, uint32_t D, uint32_t K, uint32_t H) { return D + (K - H) + j; }

// MLM_CROP_SHRINK: the capacity to shrink to — the smallest c0 * 2^k that is >= max(c0, 2 K), c0 being the capacity mlm_create gave
// the pool — or 0: leave the pool (the target is not below the current capacity)
MLM_CROP_HD long long mlm_crop_shrink_target(long long c0, long long capacity, long long K) {
    if (c0 < 1) return 0;
    long long t = c0;
    while (t < 2 * K && t < capacity) t *= 2;
    return t < capacity ? t : 0;
}

// bytes of a block's rows that a 16-byte / 4-byte / 1-byte lane path may move at once: the float plane and the byte planes of a
// pool whose blocks have `cells` voxels (rows of consecutive blocks are contiguous, so a row is aligned iff its length is)
MLM_CROP_HD int mlm_crop_float_width(int cells) { return cells % 4 == 0 ? 16 : 4; }
MLM_CROP_HD int mlm_crop_byte_width(int cells) { return cells % 16 == 0 ? 16 : cells % 4 == 0 ? 4 : 1; }
