// mlm_fuse.h — the rule of mlm_fuse_blocks (include/mlmap_hip.h): the argument check, the key checks, the predicate that says which
// rows touch the map and which create a block, and the per-voxel rule with its counts — once, for the kernels (mlm_kernels_fuse.h),
// the host driver (mlm_fuse_host.h) and the CPU test driver (tests/cpp/fuse_driver.cpp), so that all three run the very same
// arithmetic.  No reference counterpart: the reference has one map and nothing to fuse into it.
//
// The rule, per voxel.  The map holds (La, occ_a, infl_a) — 0.0f / 'u' / 'u' where it has no block — and the dump (Lb, occ_b, infl_b).
// All arithmetic is IEEE single, nothing fused.
//     clamp(x) = !(x >= lo_min) ? lo_min : (x > lo_max ? lo_max : x)           (a NaN becomes lo_min)
//     Lb' = clamp(Lb);  the voxel CONTRIBUTES iff occ_b is 'f' or 'o';  seen_a = occ_a != 'u'
//     a contributing voxel is WRITTEN in ADD, MAX and TAKE always, in FILL iff !seen_a
//     ADD: L = La + Lb'    MAX: L = seen_a ? (La > Lb' ? La : Lb') : Lb'    TAKE, FILL: L = Lb'
//     a written voxel gets log_odds = clamp(L) and occ = clamp(L) > occupied_sh ? 'o' : 'f'   (k_merge_finish's rule, not the
//     integrate path's hysteresis); any other voxel keeps its log-odds and its class bit for bit
//     with infl given and infl_b == 'o', infl_a becomes 'o' — in every mode, contributing or not
// A row TOUCHES iff it has a contributing voxel, or infl is given and it has a voxel with infl_b == 'o'.  A touching row whose block is
// absent CREATES it; the created blocks take the slots n_blocks_before + rank, rank = the created rows with a smaller row index.
#pragma once
#include <stdint.h>

#include "mlm_crop.h"

// (the values of include/mlmap_hip.h; mlm_fuse_host.h holds them to each other)
#define MLM_FUSE_M_ADD 0
#define MLM_FUSE_M_MAX 1
#define MLM_FUSE_M_TAKE 2
#define MLM_FUSE_M_FILL 3
#define MLM_FUSE_F_DRY 1
#define MLM_FUSE_F_ALL 1
#define MLM_FUSE_SUMS 12 // int64 of the summary
#define MLM_FUSE_PR 4    // int32 per row of per_row
#define MLM_FUSE_KEY_MIN (-(1 << 20)) // block keys the packed 21-bit form holds
#define MLM_FUSE_KEY_MAX ((1 << 20) - 1)

// what one voxel did (bits of mlm_fuse_voxel's result); the summary counts [4] .. [11] are the bits 0 .. 7 in this order
#define MLM_FUSE_E_CONTRIB 1u    // [4] the voxel contributes
#define MLM_FUSE_E_NEW 2u        // [5] ... and the map had not seen it
#define MLM_FUSE_E_AGREE 4u      // [6] ... both had seen it, same class
#define MLM_FUSE_E_CONFLICT 8u   // [7] ... both had seen it, different classes
#define MLM_FUSE_E_TO_O 16u      // [8] class 'o' afterwards and not before
#define MLM_FUSE_E_O_TO_F 32u    // [9] class 'o' before and 'f' afterwards
#define MLM_FUSE_E_INFL 64u      // [10] infl turned 'o'
#define MLM_FUSE_E_LO 128u       // [11] the log-odds bits changed
#define MLM_FUSE_E_OCC 256u      // (the class byte changed: a store is due)

// per_row[3]
#define MLM_FUSE_ROW_PRESENT 0
#define MLM_FUSE_ROW_CREATED 1
#define MLM_FUSE_ROW_ABSENT 2

// rowinfo flags
#define MLM_FUSE_R_TOUCH 1u // the row touches the map
#define MLM_FUSE_R_RANGE 2u // its key is outside the 21-bit range

struct MlmFuseRule {
    float lo_min, lo_max, lo_sh; // log_odds_min, log_odds_max, occupied_sh
    int32_t mode;                // MLM_FUSE_M_*
    int32_t has_infl;            // infl is given
};

// 0: fine; 1: n < 0; 2: keys, log_odds or occ null with n > 0; 3: mode outside 0..3; 4: an unknown flag bit.
// (5: a key outside the 21-bit range and 6: two rows with the same key are found over the keys themselves: mlm_fuse_key_ok, and the
// neighbours of the sorted mlm_fuse_pack values)
MLM_CROP_HD int mlm_fuse_check(long long n, const void *keys, const void *log_odds, const void *occ, int mode, int flags) {
    if (n < 0) return 1;
    if (n > 0 && (!keys || !log_odds || !occ)) return 2;
    if (mode < MLM_FUSE_M_ADD || mode > MLM_FUSE_M_FILL) return 3;
    if (flags & ~MLM_FUSE_F_ALL) return 4;
    return 0;
}
MLM_CROP_HD const char *mlm_fuse_check_text(int bad) {
    return bad == 1   ? "n must be >= 0"
           : bad == 2 ? "keys, log_odds and occ must be given"
           : bad == 3 ? "mode must be MLM_FUSE_ADD, MLM_FUSE_MAX, MLM_FUSE_TAKE or MLM_FUSE_FILL"
           : bad == 4 ? "unknown flag bit"
           : bad == 5 ? "a block key lies outside the 21-bit key range"
                      : "two rows have the same block key";
}

MLM_CROP_HD bool mlm_fuse_key_ok(int32_t kx, int32_t ky, int32_t kz) {
    return kx >= MLM_FUSE_KEY_MIN && kx <= MLM_FUSE_KEY_MAX && ky >= MLM_FUSE_KEY_MIN && ky <= MLM_FUSE_KEY_MAX && kz >= MLM_FUSE_KEY_MIN &&
           kz <= MLM_FUSE_KEY_MAX;
}
// three 21-bit biased keys, x most significant (mlm_pack_key of mlm_device.h); equal keys, equal values
MLM_CROP_HD unsigned long long mlm_fuse_pack(int32_t kx, int32_t ky, int32_t kz) {
    return ((unsigned long long)((uint32_t)(kx + (1 << 20)) & 0x1FFFFFu) << 42) | ((unsigned long long)((uint32_t)(ky + (1 << 20)) & 0x1FFFFFu) << 21) |
           (unsigned long long)((uint32_t)(kz + (1 << 20)) & 0x1FFFFFu);
}

MLM_CROP_HD bool mlm_fuse_contributes(uint8_t occ_b) { return occ_b == (uint8_t)'f' || occ_b == (uint8_t)'o'; }
// does this voxel of the dump make its row touch the map?
MLM_CROP_HD bool mlm_fuse_touches(uint8_t occ_b, bool has_infl, uint8_t infl_b) {
    return mlm_fuse_contributes(occ_b) || (has_infl && infl_b == (uint8_t)'o');
}
// ... four voxels at once: the bytes of a dword
MLM_CROP_HD bool mlm_fuse_touches4(uint32_t occ_b, bool has_infl, uint32_t infl_b) {
    bool t = false;
    for (int k = 0; k < 4; ++k) t = t || mlm_fuse_touches((uint8_t)(occ_b >> (8 * k)), has_infl, (uint8_t)(infl_b >> (8 * k)));
    return t;
}
// the row creates a block: it touches, the map does not hold its block (slot < 0) and its key is one a block can have
MLM_CROP_HD bool mlm_fuse_creates(int32_t slot, uint32_t flags) { return slot < 0 && (flags & MLM_FUSE_R_TOUCH) && !(flags & MLM_FUSE_R_RANGE); }
MLM_CROP_HD int32_t mlm_fuse_row_state(int32_t slot, uint32_t flags) {
    return slot >= 0 ? MLM_FUSE_ROW_PRESENT : mlm_fuse_creates(slot, flags) ? MLM_FUSE_ROW_CREATED : MLM_FUSE_ROW_ABSENT;
}

MLM_CROP_HD float mlm_fuse_clamp(const MlmFuseRule &R, float x) { return !(x >= R.lo_min) ? R.lo_min : (x > R.lo_max ? R.lo_max : x); }
MLM_CROP_HD uint32_t mlm_fuse_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof(u));
    return u;
}

// One voxel: (La, occ_a, infl_a) becomes what the map holds afterwards; the result says what happened (MLM_FUSE_E_*).
MLM_CROP_HD uint32_t mlm_fuse_voxel(const MlmFuseRule &R, float &La, uint8_t &occ_a, uint8_t &infl_a, float Lb, uint8_t occ_b, uint8_t infl_b) {
    uint32_t ev = 0;
    if (mlm_fuse_contributes(occ_b)) {
        const bool seen_a = occ_a != (uint8_t)'u';
        ev |= MLM_FUSE_E_CONTRIB | (!seen_a ? MLM_FUSE_E_NEW : occ_a == occ_b ? MLM_FUSE_E_AGREE : MLM_FUSE_E_CONFLICT);
        if (R.mode != MLM_FUSE_M_FILL || !seen_a) {
            const float Lc = mlm_fuse_clamp(R, Lb);
            float L = Lc;
            if (R.mode == MLM_FUSE_M_ADD) L = La + Lc;
            else if (R.mode == MLM_FUSE_M_MAX) L = seen_a ? (La > Lc ? La : Lc) : Lc;
            L = mlm_fuse_clamp(R, L);
            const uint8_t o = L > R.lo_sh ? (uint8_t)'o' : (uint8_t)'f';
            if (mlm_fuse_bits(L) != mlm_fuse_bits(La)) ev |= MLM_FUSE_E_LO;
            if (o != occ_a) ev |= MLM_FUSE_E_OCC | (o == (uint8_t)'o' ? MLM_FUSE_E_TO_O : occ_a == (uint8_t)'o' ? MLM_FUSE_E_O_TO_F : 0u);
            La = L, occ_a = o;
        }
    }
    if (R.has_infl && infl_b == (uint8_t)'o' && infl_a != (uint8_t)'o') {
        ev |= MLM_FUSE_E_INFL;
        infl_a = (uint8_t)'o';
    }
    return ev;
}
