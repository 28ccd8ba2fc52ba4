// mlm_warp.h — the rule of mlm_warp_blocks (include/mlmap_hip.h): the argument check, the gather that answers one destination voxel,
// the live predicate, the candidate rule that says which destination blocks have to be looked at and the emission order — once, for
// the kernels (mlm_kernels_warp.h), the host driver (mlm_warp_host.h) and the CPU test driver (tests/cpp/warp_driver.cpp), so that all
// three run the very same arithmetic.  No reference counterpart: the reference's map lives in one frame for good.
//
// The gather, per destination voxel v = g * n + c (block key g, cell coordinate c, n = subbox_n), all in IEEE double, nothing fused:
//     centre   p_a = (g_a * d_glb + c_a * d_sub) + d_sub_half          (subbox_id2xyz_glb_vec, as mlm_mapview.h computes it)
//     source   w   = mlm_score_world(T_sd, p)                          (mlm_score.h: five operations per axis)
//     voxel    mlm_score_voxel(w, d_sub, .)                            (floor((w / d_sub) * 1024) >> 10; invalid beyond 2^40 lattice units)
//     block / cell by floor division                                   (mlm_score_cell)
// The voxel is LIVE iff the lattice step is valid, the source block's key lies inside the 21-bit range and the block is present, and
// — with MLM_WARP_SEEN — the source voxel's occ != 'u' or its infl == 'o'.  A live voxel takes the source voxel's log_odds, occ and
// infl as they are (a released block answers from element 0 with infl 'u'); any other voxel is 0.0f / 'u' / 'u', what allocate_ram
// leaves.  T_sd is never inverted for the values.
//
// The source comes from a callable `bool src(const int g[3], const int c[3], bool new_block, float &lo, uint8_t &occ, uint8_t &infl)`:
// block index and cell coordinate of the source voxel, new_block when g differs from the previous call's (the callee keeps the block's
// slot until then: a run of voxels in one source block costs one table probe).  false: the block is absent or its key out of range.
//
// A destination block is EMITTED iff it holds a live voxel and its key lies in the call's key box (W.lo .. W.hi: the caller's box cut
// to the 21-bit range).  Emitted blocks are ordered by their packed key (mlm_warp_pack): x, then y, then z, ascending.
//
// Candidates.  Every emitted block must be looked at; the rule below names a superset.  For a present source block with key s the
// eight corners (s_a + {0, 1}) * d_glb of its cube go through the inverse transform (Ti = {R^T, -R^T o}, computed once on the host in
// double and used for nothing else); the candidates are the keys floor((min_a - d_sub) / d_glb) .. floor((max_a + d_sub) / d_glb) per
// axis, cut to the box.  Why this is complete: a live voxel's centre p maps to w = T p inside the source cube up to the rounding of
// fifteen operations; the cube is convex, so Ti w lies in the bounds of the corners' images, and p differs from Ti w by the rounding
// of both products — below 1e-6 voxel for |coordinates| < 2^30 voxels and a rigid T (|R R^T - I| <= 1e-9), against a margin of a
// whole voxel per side.  The cube's image is at most sqrt(3) d_glb wide per axis, 2 d_sub <= d_glb more with the margin (n >= 2): at
// most 4 keys per axis, 64 candidates per source block (mlm_warp_span is the bound the host sizes the candidate set by).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mlm_crop.h"
#include "mlm_score.h"

// (the values of include/mlmap_hip.h; mlm_warp_host.h holds them to each other)
#define MLM_WARP_F_SEEN 1
#define MLM_WARP_F_REPLACE 2
#define MLM_WARP_F_DRY 4
#define MLM_WARP_F_ALL 7
#define MLM_WARP_KEY_MIN (-(1 << 20)) // block keys the packed 21-bit form holds
#define MLM_WARP_KEY_MAX ((1 << 20) - 1)
#define MLM_WARP_RIGID_TOL 1e-9
#define MLM_WARP_EMPTY 0xFFFFFFFFFFFFFFFFull // no packed key: an unused entry of the candidate set

struct MlmWarpPlan {
    double T[12];         // destination frame -> source frame: R row major, then o
    double Ti[12];        // its inverse (candidate rule only)
    int32_t lo[3], hi[3]; // emitted keys per axis, inclusive: the key box within the 21-bit range (lo > hi: nothing)
    int32_t seen;         // MLM_WARP_SEEN
};

struct MlmWarpGeom {
    double d_sub, d_glb, d_sub_half;
    int n;
};

// 0: fine (W is filled); 1: no transform; 2: a non-finite entry; 3: not rigid; 4: one of key_lo / key_dims null and the other not;
// 5: a key dim < 1; 6: key_lo + key_dims beyond int32; 7: an unknown flag bit; 8: cap < 0
MLM_RW_HD int mlm_warp_check(const double *T, const int32_t *key_lo, const int32_t *key_dims, int flags, long long cap, MlmWarpPlan &W) {
    if (!T) return 1;
    for (int i = 0; i < 12; ++i)
        if (!(fabs(T[i]) <= 1.7976931348623157e308)) return 2; // (NaN fails)
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double s = (T[3 * a] * T[3 * b] + T[3 * a + 1] * T[3 * b + 1]) + T[3 * a + 2] * T[3 * b + 2];
            if (!(fabs(s - (a == b ? 1.0 : 0.0)) <= MLM_WARP_RIGID_TOL)) return 3;
        }
    if ((key_lo == nullptr) != (key_dims == nullptr)) return 4;
    MlmCropBox B{};
    if (key_lo) {
        const int bad = mlm_crop_check(key_lo, key_dims, 0, 0, B);
        if (bad) return bad == 2 ? 5 : 6;
    }
    if (flags & ~MLM_WARP_F_ALL) return 7;
    if (cap < 0) return 8;
    for (int i = 0; i < 12; ++i) W.T[i] = T[i];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) W.Ti[3 * a + b] = T[3 * b + a];
        W.Ti[9 + a] = -((T[a] * T[9] + T[3 + a] * T[10]) + T[6 + a] * T[11]);
        W.lo[a] = key_lo && B.lo[a] > MLM_WARP_KEY_MIN ? B.lo[a] : MLM_WARP_KEY_MIN;
        W.hi[a] = key_lo && B.hi[a] < MLM_WARP_KEY_MAX ? B.hi[a] : MLM_WARP_KEY_MAX;
    }
    W.seen = (flags & MLM_WARP_F_SEEN) ? 1 : 0;
    return 0;
}
MLM_RW_HD const char *mlm_warp_check_text(int bad) {
    return bad == 1   ? "null transform"
           : bad == 2 ? "the transform has a non-finite entry"
           : bad == 3 ? "the transform is not rigid: max |R R^T - I| > 1e-9"
           : bad == 4 ? "key_lo and key_dims must be given together"
           : bad == 5 ? "key_dims must be >= 1"
           : bad == 6 ? "key_lo + key_dims must fit an int32"
           : bad == 7 ? "unknown flag bit"
                      : "cap must be >= 0";
}

MLM_RW_HD bool mlm_warp_key_ok(const int g[3]) {
    return g[0] >= MLM_WARP_KEY_MIN && g[0] <= MLM_WARP_KEY_MAX && g[1] >= MLM_WARP_KEY_MIN && g[1] <= MLM_WARP_KEY_MAX && g[2] >= MLM_WARP_KEY_MIN &&
           g[2] <= MLM_WARP_KEY_MAX;
}
MLM_RW_HD bool mlm_warp_in_box(const MlmWarpPlan &W, const int g[3]) {
    return g[0] >= W.lo[0] && g[0] <= W.hi[0] && g[1] >= W.lo[1] && g[1] <= W.hi[1] && g[2] >= W.lo[2] && g[2] <= W.hi[2];
}
// the emission order: three 21-bit biased keys, x most significant (mlm_pack_key of mlm_device.h)
MLM_RW_HD unsigned long long mlm_warp_pack(const int g[3]) {
    return ((unsigned long long)((uint32_t)(g[0] + (1 << 20)) & 0x1FFFFFu) << 42) | ((unsigned long long)((uint32_t)(g[1] + (1 << 20)) & 0x1FFFFFu) << 21) |
           (unsigned long long)((uint32_t)(g[2] + (1 << 20)) & 0x1FFFFFu);
}
MLM_RW_HD void mlm_warp_unpack(unsigned long long key, int g[3]) {
    g[0] = (int)((key >> 42) & 0x1FFFFFu) - (1 << 20);
    g[1] = (int)((key >> 21) & 0x1FFFFFu) - (1 << 20);
    g[2] = (int)(key & 0x1FFFFFu) - (1 << 20);
}

// the source voxel of destination voxel (g, c); false: the lattice step is invalid
MLM_RW_HD bool mlm_warp_source(const double T[12], const MlmWarpGeom &G, const int g[3], const int c[3], int32_t v[3]) {
    double p[3], w[3];
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) p[a] = (g[a] * G.d_glb + c[a] * G.d_sub) + G.d_sub_half;
    mlm_score_world(T, p, w);
    return mlm_score_voxel(w, G.d_sub, v);
}

// One destination voxel: true iff live; lo / occ / infl are its answer either way.  B: the source block of this caller's previous
// voxel (MlmScoreBlock{} at first).
template <class Src>
MLM_RW_HD bool mlm_warp_voxel(const double T[12], bool seen, const MlmWarpGeom &G, const int g[3], const int c[3], Src &src, MlmScoreBlock &B, float &lo,
                              uint8_t &occ, uint8_t &infl) {
    lo = 0.0f, occ = (uint8_t)'u', infl = (uint8_t)'u';
    int32_t v[3];
    if (!mlm_warp_source(T, G, g, c, v)) return false;
    int sc[3];
    const bool nb = mlm_score_cell(v, G.n, B, sc);
    float L = 0.0f;
    uint8_t o = (uint8_t)'u', i = (uint8_t)'u';
    if (!src(B.g, sc, nb, L, o, i)) return false;
    if (seen && o == (uint8_t)'u' && i != (uint8_t)'o') return false;
    lo = L, occ = o, infl = i;
    return true;
}

// The candidate keys of the present source block s: klo .. khi per axis (inclusive); false: none inside the box.
MLM_RW_HD bool mlm_warp_candidates(const MlmWarpPlan &W, const MlmWarpGeom &G, const int s[3], int32_t klo[3], int32_t khi[3]) {
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int k = 0; k < 8; ++k) {
        const double q[3] = {(s[0] + (k & 1)) * G.d_glb, (s[1] + ((k >> 1) & 1)) * G.d_glb, (s[2] + (k >> 2)) * G.d_glb};
        double w[3];
        mlm_score_world(W.Ti, q, w);
        MLM_RW_UNROLL
        for (int a = 0; a < 3; ++a) {
            if (!(fabs(w[a]) < 1e300)) return false; // (not finite, or far beyond every key: no centre of a keyed block maps here)
            mn[a] = k == 0 || w[a] < mn[a] ? w[a] : mn[a];
            mx[a] = k == 0 || w[a] > mx[a] ? w[a] : mx[a];
        }
    }
    bool any = true;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        double fl = floor((mn[a] - G.d_sub) / G.d_glb), fh = floor((mx[a] + G.d_sub) / G.d_glb);
        if (fl < (double)W.lo[a]) fl = (double)W.lo[a];
        if (fh > (double)W.hi[a]) fh = (double)W.hi[a];
        any = any && fl <= fh;
        klo[a] = any ? (int32_t)fl : 0;
        khi[a] = any ? (int32_t)fh : -1;
    }
    return any;
}

// most candidate keys per axis of any source block under Ti (the bound above from |R^T| row sums; the host sizes the candidate set
// by the product): an interval of length e in units of d_glb meets at most floor(e) + 2 keys
MLM_RW_HD int mlm_warp_span(const MlmWarpPlan &W, const MlmWarpGeom &G, int a) {
    const double e = ((fabs(W.Ti[3 * a]) + fabs(W.Ti[3 * a + 1])) + fabs(W.Ti[3 * a + 2])) + 2.0 * G.d_sub / G.d_glb;
    return (int)floor(e + 1e-6) + 2;
}

// cell coordinate (x fastest) of cell index i < n^3 by two divisions by n — the callers pass their own divider
template <class Div> MLM_RW_HD void mlm_warp_cell(uint32_t i, int n, Div div, int c[3]) {
    const uint32_t q = div(i), r = div(q);
    c[0] = (int)(i - q * (uint32_t)n);
    c[1] = (int)(q - r * (uint32_t)n);
    c[2] = (int)r;
}
