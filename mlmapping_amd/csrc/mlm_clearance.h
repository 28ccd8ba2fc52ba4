// mlm_clearance.h — the segment walk through a distance field of mlm_query_clearance (include/mlmap_hip.h): the per-ray walk and the
// per-group reduction, once, for the kernels (mlm_kernels_clearance.h), the host branch of the entry point (mlmap_hip.hip) and the CPU
// test driver (tests/cpp/clearance_driver.cpp), so that all three run the very same control flow.  No reference counterpart: the
// reference has no segment query and no distance field; the path is mlm_query_rays' (mlm_raywalk.h, walked here with a block edge of 1,
// which makes MlmRayState::g the absolute voxel and folds the block division away), the field is what mlm_export_esdf wrote.
//
// The rule (u_0 .. u_N the path, f(v) = min(max(sqdist[v], 0), sq_cap) inside the box; outside the box the walk ends with status
// MLM_CLEAR_LEFT, or, with MLM_CLEAR_OUTSIDE_PASS, f(v) = sq_cap): the walk stops at the smallest K whose voxel has left the box
// (status 2) or has f(u_K) <= sq_stop (status 1); K = N + 1 and status 0 without one.  Passed = u_0 .. u_{K-1}; seen = passed, plus
// u_K at status 1.  min_sq / min3: the minimum of f over seen and the seen voxel of smallest path index attaining it; cost: the sum of
// sq_cap - f over passed (at most (3 * 2^15 + 1) * 2^20 < 2^38); n_near: the passed voxels with f < sq_cap.
//
// Everything but the lattice conversion of mlm_raywalk.h is integer code without a runtime division.  The place of the current voxel
// in the field is kept incrementally: per axis the coordinate relative to lo (64 bits: |v| <= 2^30 against any int32 lo), tested by one
// unsigned compare against dims, and the linear index moved by the stride of the axis stepped, in 64 bits modulo 2^64 — inside the box
// it is the true index (below 2^31: mlm_box_check), outside it is never used.
//
// Look-ahead.  The path does not depend on what is read (mlm_query_rays' does not either, but there a block's class can end the memory
// traffic of many steps; here every voxel costs one load).  mlm_clear_walk<K> therefore steps the walk K voxels ahead, issues their K
// loads together, and only then tests them in path order; what lies behind the stop is discarded, so the answer is K's whatever K is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlm_raywalk.h"

#define MLM_CLEAR_WORDS 8           // MLM_CLEAR_ROW of the header
#define MLM_CLEAR_MAX_SQ (1 << 20)  // largest sq_stop and sq_cap
#define MLM_CLEAR_NO_MIN (-1)       // MLM_CLEAR_NONE of the header
#define MLM_CLEAR_STATUS_LEFT 2     // MLM_CLEAR_LEFT of the header

// the field of a call: one int32 per voxel of the box lo <= v < lo + dims, [dims[2]][dims[1]][dims[0]]
struct MlmClearField {
    const int32_t *sqdist;
    int32_t lo[3], dims[3];
    int32_t sq_stop, sq_cap;
    int32_t outside_pass; // MLM_CLEAR_OUTSIDE_PASS
};

struct MlmClearResult {
    int status;     // 1 stopped by the field, 2 left the box, 0 reached the end, -1 invalid ray
    int voxel[3];   // u_K, or the end voxel
    double t;       // segment parameter at which u_K is entered (0 at the start voxel); 1 at status 0
    int n_steps;    // K
    int min_sq;     // MLM_CLEAR_NO_MIN: no voxel seen
    int min3[3];
    long long cost;
    int n_near;
};

// where the walk stands in the field
struct MlmClearPlace {
    long long rel[3];         // voxel - lo
    unsigned long long idx;   // (rel[2] * dims[1] + rel[1]) * dims[0] + rel[0] modulo 2^64
};

MLM_RW_HD void mlm_clear_invalid(MlmClearResult &o) {
    o.status = -1;
    o.voxel[0] = o.voxel[1] = o.voxel[2] = 0;
    o.t = 0.0;
    o.n_steps = 0;
    o.min_sq = MLM_CLEAR_NO_MIN;
    o.min3[0] = o.min3[1] = o.min3[2] = 0;
    o.cost = 0;
    o.n_near = 0;
}

MLM_RW_HD void mlm_clear_place(const MlmClearField &F, const int v[3], MlmClearPlace &W) {
    // (constant indices, as in mlm_score_in_box: the field's box is kernel-argument data and has to stay in scalar registers)
    W.rel[0] = (long long)v[0] - F.lo[0];
    W.rel[1] = (long long)v[1] - F.lo[1];
    W.rel[2] = (long long)v[2] - F.lo[2];
    W.idx = ((unsigned long long)W.rel[2] * (unsigned long long)F.dims[1] + (unsigned long long)W.rel[1]) * (unsigned long long)F.dims[0] +
            (unsigned long long)W.rel[0];
}

MLM_RW_HD bool mlm_clear_in_box(const MlmClearField &F, const MlmClearPlace &W) {
    return (unsigned long long)W.rel[0] < (unsigned long long)F.dims[0] && (unsigned long long)W.rel[1] < (unsigned long long)F.dims[1] &&
           (unsigned long long)W.rel[2] < (unsigned long long)F.dims[2];
}

// one step of the path and of the place; m_in / d_in: the parameter at which the new voxel is entered
MLM_RW_HD void mlm_clear_step(const MlmClearField &F, MlmRayState &S, MlmClearPlace &W, int &m_in, int &d_in) {
    const int r0 = S.r[0], r1 = S.r[1], r2 = S.r[2];
    mlm_ray_step(S, 1, m_in, d_in);
    // the axis stepped is the one whose count went down; its stride: 1, dims[0], dims[0] * dims[1]
    const long long s0 = r0 != S.r[0] ? S.s[0] : 0, s1 = r1 != S.r[1] ? S.s[1] : 0, s2 = r2 != S.r[2] ? S.s[2] : 0;
    W.rel[0] += s0;
    W.rel[1] += s1;
    W.rel[2] += s2;
    W.idx += (unsigned long long)s0 + (unsigned long long)s1 * (unsigned long long)F.dims[0] +
             (unsigned long long)s2 * ((unsigned long long)F.dims[0] * (unsigned long long)F.dims[1]);
}

// min(max(s, 0), cap)
MLM_RW_HD int32_t mlm_clear_clamp(int32_t s, int32_t cap) { return s < 0 ? 0 : (s > cap ? cap : s); }

// The whole walk of one ray, K voxels looked ahead (K >= 1).  d = subbox_d_xyz.
template <int K> MLM_RW_HD void mlm_clear_walk(const double p0[3], const double p1[3], double d, const MlmClearField &F, MlmClearResult &o) {
    MlmRayState S;
    if (!mlm_ray_setup(p0, p1, d, 1, S)) {
        mlm_clear_invalid(o);
        return;
    }
    MlmClearPlace W;
    mlm_clear_place(F, S.g, W);
    int m_in = 0, d_in = 1; // of the voxel the walk stands on
    bool have = true;       // the walk stands on a path voxel that has not been taken into a batch yet
    int k = 0, status = 0, near = 0, mn = MLM_CLEAR_NO_MIN;
    int mv0 = 0, mv1 = 0, mv2 = 0, lv0 = S.g[0], lv1 = S.g[1], lv2 = S.g[2], lm = 0, ld = 1;
    long long cost = 0;
    while (have && status == 0) {
        // the next K path voxels (fewer at the end of the path): voxel, entry parameter, whether in the box, and the field there
        int vx[K], vy[K], vz[K], em[K], ed[K];
        int32_t raw[K];
        bool in[K], on[K];
        MLM_RW_UNROLL
        for (int j = 0; j < K; ++j) {
            on[j] = have;
            in[j] = false;
            raw[j] = 0;
            vx[j] = vy[j] = vz[j] = 0;
            em[j] = 0, ed[j] = 1;
            if (have) {
                vx[j] = S.g[0], vy[j] = S.g[1], vz[j] = S.g[2];
                em[j] = m_in, ed[j] = d_in;
                in[j] = mlm_clear_in_box(F, W);
                if (in[j]) raw[j] = F.sqdist[W.idx];
                have = (S.r[0] | S.r[1] | S.r[2]) != 0;
                if (have) mlm_clear_step(F, S, W, m_in, d_in);
            }
        }
        // ... tested in path order; behind a stop nothing counts
        MLM_RW_UNROLL
        for (int j = 0; j < K; ++j) {
            if (!on[j] || status != 0) continue;
            lv0 = vx[j], lv1 = vy[j], lv2 = vz[j];
            lm = em[j], ld = ed[j];
            if (!in[j] && !F.outside_pass) {
                status = MLM_CLEAR_STATUS_LEFT;
                continue;
            }
            const int f = in[j] ? mlm_clear_clamp(raw[j], F.sq_cap) : F.sq_cap;
            if (f <= F.sq_stop) status = 1;
            if (mn == MLM_CLEAR_NO_MIN || f < mn) { // (seen: passed, and the voxel of a stop by the field)
                mn = f;
                mv0 = vx[j], mv1 = vy[j], mv2 = vz[j];
            }
            if (status == 0) {
                cost += (long long)(F.sq_cap - f);
                near += f < F.sq_cap ? 1 : 0;
                ++k;
            }
        }
    }
    o.status = status;
    o.voxel[0] = lv0, o.voxel[1] = lv1, o.voxel[2] = lv2;
    o.t = status ? (double)lm / (double)ld : 1.0; // (the start voxel: 0 / 1)
    o.n_steps = k;
    o.min_sq = mn;
    o.min3[0] = mv0, o.min3[1] = mv1, o.min3[2] = mv2;
    o.cost = cost;
    o.n_near = near;
}

// The row of one group: the segments [begin, end) of the batch, from the five per-ray words the rows need.
MLM_RW_HD void mlm_clear_group(int begin, int end, const int8_t *status, const int32_t *min_sq, const int64_t *cost, const int32_t *n_steps,
                               const int32_t *n_near, int64_t row[MLM_CLEAR_WORDS]) {
    long long first = -1, st = 0, mn = -1, at = -1, c = 0, ns = 0, nn = 0;
    for (int i = begin; i < end; ++i) {
        const int32_t m = min_sq[i];
        if (m != MLM_CLEAR_NO_MIN && (mn < 0 || m < mn)) {
            mn = m;
            at = i - begin;
        }
        c += cost[i];
        ns += n_steps[i];
        nn += n_near[i];
        if (status[i] != 0) { // the first segment that does not reach its end closes the group's count
            first = i - begin;
            st = status[i];
            break;
        }
    }
    row[0] = (int64_t)end - begin;
    row[1] = first;
    row[2] = st;
    row[3] = mn;
    row[4] = at;
    row[5] = c;
    row[6] = ns;
    row[7] = nn;
}
