// mlm_age.h — the rule of mlm_age_blocks (include/mlmap_hip.h): the argument check, the predicate that says which blocks a call
// selects, the per-voxel rule with its counts and the "this voxel leaves its block empty" predicate — once, for the kernel
// (mlm_kernels_age.h), the host driver (mlm_age_host.h) and the CPU test driver (tests/cpp/age_driver.cpp), so that all three run the
// very same arithmetic.  No reference counterpart: the reference's observed_group_map only ever accumulates evidence.
//
// The rule, per voxel (La, occ_a, infl_a) of a selected block.  All arithmetic is IEEE single, nothing fused, subnormals kept.
//     clamp(x) = mlm_fuse_clamp: !(x >= lo_min) ? lo_min : (x > lo_max ? lo_max : x)           (a NaN becomes lo_min)
//     the voxel is AGED iff occ_a != 'u' or (bits(La) & 0x7fffffff) != 0      (it holds a class or evidence; +-0.0f / 'u' is not aged)
//     SCALE: L = La * amount        STEP: L = La > amount ? La - amount : (La < -amount ? La + amount : 0.0f)
//     L = clamp(L)
//     with FORGET and fabsf(L) <= forget the voxel is FORGOTTEN: log-odds +0.0f, occ 'u'
//     otherwise occ = occ_a != 'u' ? (L > occupied_sh ? 'o' : 'f') : 'u'     (mlm_fuse_blocks' and k_merge_finish's rule; evidence
//     that never reached a class decays but is never classified), log-odds = L
//     with CLEAR_INFL the infl of every voxel of the block, aged or not, becomes 'u'; otherwise infl is untouched
// A voxel is EMPTY afterwards iff occ == 'u', infl != 'o' and (bits(L) & 0x7fffffff) == 0; a selected block all of whose voxels are
// empty is EMPTY, and MLM_AGE_DROP drops the empty selected blocks by mlm_crop.h's hole filling over that set.
#pragma once
#include <stdint.h>

#include "mlm_fuse.h"

// (the values of include/mlmap_hip.h; mlm_age_host.h holds them to each other)
#define MLM_AGE_M_SCALE 0
#define MLM_AGE_M_STEP 1
#define MLM_AGE_F_OUTSIDE 1
#define MLM_AGE_F_DRY 2
#define MLM_AGE_F_FORGET 4
#define MLM_AGE_F_DROP 8
#define MLM_AGE_F_CLEAR_INFL 16
#define MLM_AGE_F_ALL 31
#define MLM_AGE_SUMS 12 // int64 of the summary
#define MLM_AGE_PB 4    // int32 per block of per_block

// what one voxel did (bits of mlm_age_voxel's result); the summary counts [4] .. [11] are the bits 0 .. 7 in this order
#define MLM_AGE_E_AGED 1u      // [4] the voxel is aged
#define MLM_AGE_E_LO 2u        // [5] its log-odds bits changed
#define MLM_AGE_E_FORGOT 4u    // [6] it was forgotten
#define MLM_AGE_E_FORGOT_O 8u  // [7] ... and its class was 'o'
#define MLM_AGE_E_FORGOT_F 16u // [8] ... and its class was 'f'
#define MLM_AGE_E_O_TO_F 32u   // [9] class 'o' before and 'f' afterwards
#define MLM_AGE_E_F_TO_O 64u   // [10] class 'f' before and 'o' afterwards
#define MLM_AGE_E_INFL 128u    // [11] infl went 'o' -> 'u'
#define MLM_AGE_E_OCC 256u     // (the class byte changed: a store is due)
#define MLM_AGE_E_INFL_ST 512u // (the infl byte changed: a store is due)

// per_block[3]
#define MLM_AGE_B_UNSELECTED 0
#define MLM_AGE_B_KEPT 1
#define MLM_AGE_B_EMPTY 2 // selected and empty afterwards: dropped with MLM_AGE_DROP, "would be dropped" otherwise

struct MlmAgeRule {
    MlmFuseRule R;        // log_odds_min, log_odds_max, occupied_sh (mode and has_infl unused)
    int32_t mode;         // MLM_AGE_M_*
    int32_t flags;        // MLM_AGE_F_*
    float amount, forget; // forget is read with MLM_AGE_F_FORGET only
};

// which blocks a call selects: every block (all != 0), or those whose key lies inside B (B.inside = 1) or outside it (B.inside = 0)
struct MlmAgeSel {
    MlmCropBox B;
    int32_t all;
};

MLM_CROP_HD bool mlm_age_finite(float x) { return (mlm_fuse_bits(x) & 0x7F800000u) != 0x7F800000u; }

// 0: fine (S is filled); 1: one of key_lo / key_dims null and the other not; 2: a key dim < 1; 3: key_lo + key_dims beyond int32
// (mlm_crop_check's 2 and 3, with its texts); 4: an unknown flag bit; 5: mode outside 0..1; 6: a non-finite amount; 7: SCALE with
// amount outside [0, 1]; 8: STEP with amount < 0; 9: FORGET with a non-finite or negative forget
MLM_CROP_HD int mlm_age_check(const int32_t *key_lo, const int32_t *key_dims, int mode, float amount, float forget, int flags, MlmAgeSel &S) {
    if ((key_lo == nullptr) != (key_dims == nullptr)) return 1;
    S.all = key_lo ? 0 : 1;
    if (key_lo) {
        const int bad = mlm_crop_check(key_lo, key_dims, 0, 0, S.B);
        if (bad) return bad; // (2 or 3: the box is given, no flag, cap 0)
    } else {
        for (int a = 0; a < 3; ++a) S.B.lo[a] = S.B.hi[a] = 0;
    }
    if (flags & ~MLM_AGE_F_ALL) return 4;
    S.B.inside = (flags & MLM_AGE_F_OUTSIDE) ? 0 : 1;
    if (mode < MLM_AGE_M_SCALE || mode > MLM_AGE_M_STEP) return 5;
    if (!mlm_age_finite(amount)) return 6;
    if (mode == MLM_AGE_M_SCALE && !(amount >= 0.0f && amount <= 1.0f)) return 7;
    if (mode == MLM_AGE_M_STEP && amount < 0.0f) return 8;
    if ((flags & MLM_AGE_F_FORGET) && (!mlm_age_finite(forget) || forget < 0.0f)) return 9;
    return 0;
}
MLM_CROP_HD const char *mlm_age_check_text(int bad) {
    return bad == 1   ? "key_lo and key_dims must be given together"
           : bad <= 4 ? mlm_crop_check_text(bad)
           : bad == 5 ? "mode must be MLM_AGE_SCALE or MLM_AGE_STEP"
           : bad == 6 ? "amount must be finite"
           : bad == 7 ? "MLM_AGE_SCALE takes an amount in [0, 1]"
           : bad == 8 ? "MLM_AGE_STEP takes an amount >= 0"
                      : "MLM_AGE_FORGET takes a finite forget >= 0";
}

// is the block with this key selected?
MLM_CROP_HD bool mlm_age_selects(const MlmAgeSel &S, int32_t kx, int32_t ky, int32_t kz) { return S.all != 0 || mlm_crop_drops(S.B, kx, ky, kz); }

// does this voxel leave its block non-empty?
MLM_CROP_HD bool mlm_age_voxel_empty(float L, uint8_t occ, uint8_t infl) {
    return occ == (uint8_t)'u' && infl != (uint8_t)'o' && (mlm_fuse_bits(L) & 0x7FFFFFFFu) == 0u;
}

// One voxel of a selected block: (La, occ_a, infl_a) becomes what the map holds afterwards; the result says what happened (MLM_AGE_E_*).
MLM_CROP_HD uint32_t mlm_age_voxel(const MlmAgeRule &A, float &La, uint8_t &occ_a, uint8_t &infl_a) {
    uint32_t ev = 0;
    if (occ_a != (uint8_t)'u' || (mlm_fuse_bits(La) & 0x7FFFFFFFu) != 0u) {
        ev |= MLM_AGE_E_AGED;
        float L;
        if (A.mode == MLM_AGE_M_SCALE) L = La * A.amount;
        else L = La > A.amount ? La - A.amount : (La < -A.amount ? La + A.amount : 0.0f);
        L = mlm_fuse_clamp(A.R, L);
        uint8_t o = occ_a;
        if ((A.flags & MLM_AGE_F_FORGET) && __builtin_fabsf(L) <= A.forget) {
            ev |= MLM_AGE_E_FORGOT | (occ_a == (uint8_t)'o' ? MLM_AGE_E_FORGOT_O : occ_a == (uint8_t)'f' ? MLM_AGE_E_FORGOT_F : 0u);
            L = 0.0f, o = (uint8_t)'u';
        } else if (occ_a != (uint8_t)'u') {
            o = L > A.R.lo_sh ? (uint8_t)'o' : (uint8_t)'f';
            if (occ_a == (uint8_t)'o' && o == (uint8_t)'f') ev |= MLM_AGE_E_O_TO_F;
            if (occ_a == (uint8_t)'f' && o == (uint8_t)'o') ev |= MLM_AGE_E_F_TO_O;
        }
        if (mlm_fuse_bits(L) != mlm_fuse_bits(La)) ev |= MLM_AGE_E_LO;
        if (o != occ_a) ev |= MLM_AGE_E_OCC;
        La = L, occ_a = o;
    }
    if ((A.flags & MLM_AGE_F_CLEAR_INFL) && infl_a != (uint8_t)'u') {
        ev |= MLM_AGE_E_INFL_ST | (infl_a == (uint8_t)'o' ? MLM_AGE_E_INFL : 0u);
        infl_a = (uint8_t)'u';
    }
    return ev;
}
