// mlm_sweep.h — the swept ball of mlm_query_sweeps (include/mlmap_hip.h): the column table of a radius, the hit key whose unsigned
// minimum is the contract's tie rule, and the walk, once, for the kernel (mlm_kernels_sweeps.h), the host mirror (MapView::sweep,
// mlm_mapview.h) and the CPU test driver (tests/cpp/sweep_driver.cpp), so that all three run the very same control flow.  No reference
// counterpart: the reference has no segment query; the path is mlm_raywalk.h's, the classes are those of the reference's point queries.
//
// The rule.  A step goes from u_{k-1} to u_k = u_{k-1} + s e_a.  The balls around u_0 .. u_{k-1} held no obstacle, so only
// B(u_k) \ B(u_{k-1}) can hold one.  Take a column (p, q) of the two other axes (b < c) with p^2 + q^2 <= r^2: along a the ball is the
// interval [-m, m], m = isqrt(r^2 - p^2 - q^2), so the difference holds exactly ONE voxel of the column, u_k + s m e_a + p e_b + q e_c —
// the cap, L(r) voxels per step instead of (2r + 1)^3.  Every obstacle of B(u_k) lies in the cap, so the minimum of the hit key over
// the cap is the minimum over the ball.  Only the start voxel needs the full ball: mlm_near_best (mlm_nearest.h) at the centre of u_0
// with C = r, where E = 2^20 |o - u_0|^2 and the tie order is the same.
//
// The table of a radius: rows q = -r .. r, in each the columns p = -w .. w, w = isqrt(r^2 - q^2); one word per column,
// (p + 16) | (q + 16) << 6 | m << 12 | (m^2 + p^2 + q^2) << 18.
//
// The voxels come from a callable with three members (wave-uniform arguments and results on the device):
//     int centre(const int g[3], const int c[3], bool new_block)
//         the MLM_SWEEP_* bits that hold at the path voxel (mlm_raywalk.h's callable; INFL is needed at radius 0 only);
//     unsigned long long start(const MlmRayState &S, int r, int flags)
//         r >= 1: the smallest key over the full ball around the start voxel (mlm_sweep_start), MLM_SWEEP_NOKEY if it is empty;
//     unsigned long long cap(const MlmRayState &S, int axis, int s, bool new_block, int r, int flags)
//         r >= 1: the smallest key over the cap of the step just taken (S is at u_k), MLM_SWEEP_NOKEY if it is empty.
// start and cap are not called with flags == 0: nothing stops such a ray.
#pragma once
#include <stdint.h>

#include "mlm_nearest.h"
#include "mlm_raywalk.h"

#define MLM_SWEEP_MAX_R 16
#define MLM_SWEEP_MAX_COLS 797 // L(16)
#define MLM_SWEEP_NOKEY 0xFFFFFFFFFFFFFFFFull

struct MlmSweepResult {
    MlmRayResult ray; // status, the ball's centre voxel (or the end voxel), t, n_steps, n_unknown: mlm_query_rays' meaning
    int hit[3];       // the obstacle voxel responsible; the end voxel without a stop; 0 for an invalid ray
    int hit_sq;       // |hit - voxel|^2, or -1
};

MLM_RW_HD int mlm_sweep_isqrt(int v) { // v <= 256
    int m = 0;
    while ((m + 1) * (m + 1) <= v) ++m;
    return m;
}
// half width of row q (|q| <= r), and the index of its first column
MLM_RW_HD int mlm_sweep_row_half(int r, int q) { return mlm_sweep_isqrt(r * r - q * q); }
MLM_RW_HD int mlm_sweep_row_begin(int r, int q) {
    int at = 0;
    for (int u = -r; u < q; ++u) at += 2 * mlm_sweep_row_half(r, u) + 1;
    return at;
}
MLM_RW_HD uint32_t mlm_sweep_column(int r, int p, int q) {
    const int lat = p * p + q * q, m = mlm_sweep_isqrt(r * r - lat);
    return (uint32_t)(p + 16) | (uint32_t)(q + 16) << 6 | (uint32_t)m << 12 | (uint32_t)(m * m + lat) << 18;
}
// L(r)
MLM_RW_HD int mlm_sweep_columns(int r) { return mlm_sweep_row_begin(r, r + 1); }
// the whole table (tab: L(r) <= MLM_SWEEP_MAX_COLS words); returns L(r)
MLM_RW_HD int mlm_sweep_table(int r, uint32_t *tab) {
    int at = 0;
    for (int q = -r; q <= r; ++q) {
        const int w = mlm_sweep_row_half(r, q);
        for (int p = -w; p <= w; ++p) tab[at++] = mlm_sweep_column(r, p, q);
    }
    return at;
}

// the voxel of a column in the cap of a step along `axis` with sign s, relative to u_k (no indexing by axis: registers)
MLM_RW_HD void mlm_sweep_offset(uint32_t col, int axis, int s, int off[3]) {
    const int p = (int)(col & 63u) - 16, q = (int)((col >> 6) & 63u) - 16, m = s * (int)((col >> 12) & 31u);
    off[0] = axis == 0 ? m : p;
    off[1] = axis == 1 ? m : (axis == 0 ? p : q);
    off[2] = axis == 2 ? m : q;
}
// sq * 2^24 + (dz + 64) * 2^16 + (dy + 64) * 2^8 + (dx + 64): smallest (sq, z, y, x) first, mlm_query_nearest's tie rule
MLM_RW_HD unsigned long long mlm_sweep_key(int sq, const int off[3]) {
    return ((unsigned long long)(uint32_t)sq << 24) | ((unsigned long long)(uint32_t)(off[2] + 64) << 16) | ((unsigned long long)(uint32_t)(off[1] + 64) << 8) |
           (unsigned long long)(uint32_t)(off[0] + 64);
}
MLM_RW_HD unsigned long long mlm_sweep_column_key(uint32_t col, int axis, int s, int off[3]) {
    mlm_sweep_offset(col, axis, s, off);
    return mlm_sweep_key((int)(col >> 18), off);
}

// The full ball around voxel v (r >= 1) through mlm_nearest.h's search: a point at the centre of v, C = r.  near: mlm_nearest.h's callable.
template <class Near> MLM_RW_HD unsigned long long mlm_sweep_start(const int v[3], int n, int r, int flags, Near &near) {
    MlmNearPoint p;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        p.v[a] = v[a];
        p.r[a] = 512;
    }
    p.lim = (long long)(1024 * r) * (1024 * r);
    p.C = r;
    const unsigned long long key = mlm_near_best(p, n, flags, near);
    if (key == MLM_NEAR_NOKEY) return MLM_SWEEP_NOKEY;
    return ((key >> 44) << 24) | (key & 0xFFFFFFull); // (E = 2^20 |o - v|^2; the offsets are packed alike)
}

// The whole contract for one segment.  n = subbox_n, d = subbox_d_xyz, r = radius in voxels.
template <class Vox>
MLM_RW_HD void mlm_sweep_walk(const double p0[3], const double p1[3], double d, int n, int r, int flags, Vox &vox, MlmSweepResult &o) {
    MlmRayState S;
    if (!mlm_ray_setup(p0, p1, d, n, S)) {
        mlm_ray_invalid(o.ray);
        o.hit[0] = o.hit[1] = o.hit[2] = 0;
        o.hit_sq = -1;
        return;
    }
    const int zero[3] = {0, 0, 0};
    const unsigned long long own = mlm_sweep_key(0, zero); // radius 0: the path voxel itself
    int k = 0, unk = 0, m_in = 0, d_in = 1;
    int bits = vox.centre(S.g, S.c, true);
    unsigned long long key = MLM_SWEEP_NOKEY;
    if (flags) key = r == 0 ? ((bits & flags) ? own : MLM_SWEEP_NOKEY) : vox.start(S, r, flags);
    for (;;) {
        if (key != MLM_SWEEP_NOKEY) break;
        unk += (bits >> 2) & 1;
        ++k;
        if ((S.r[0] | S.r[1] | S.r[2]) == 0) break;
        const int r0 = S.r[0], r1 = S.r[1];
        const bool nb = mlm_ray_step(S, n, m_in, d_in);
        const int axis = S.r[0] != r0 ? 0 : (S.r[1] != r1 ? 1 : 2);
        const int s = axis == 0 ? S.s[0] : (axis == 1 ? S.s[1] : S.s[2]);
        bits = vox.centre(S.g, S.c, nb);
        if (flags) key = r == 0 ? ((bits & flags) ? own : MLM_SWEEP_NOKEY) : vox.cap(S, axis, s, nb, r, flags);
    }
    const bool stopped = key != MLM_SWEEP_NOKEY;
    o.ray.status = stopped ? 1 : 0;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) o.ray.voxel[a] = S.g[a] * n + S.c[a];
    o.ray.t = stopped ? (double)m_in / (double)d_in : 1.0; // (the start voxel: 0 / 1)
    o.ray.n_steps = k;
    o.ray.n_unknown = unk;
    o.hit[0] = o.ray.voxel[0] + (stopped ? (int)(key & 255u) - 64 : 0);
    o.hit[1] = o.ray.voxel[1] + (stopped ? (int)((key >> 8) & 255u) - 64 : 0);
    o.hit[2] = o.ray.voxel[2] + (stopped ? (int)((key >> 16) & 255u) - 64 : 0);
    o.hit_sq = stopped ? (int)(key >> 24) : -1;
}
