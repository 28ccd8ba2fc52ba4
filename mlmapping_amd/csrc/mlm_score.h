// mlm_score.h — the scan-to-map score of mlm_score_poses (include/mlmap_hip.h): the transform of a sensor-frame point by a pose, the
// lattice step and its validity test, the box test and the cost of a distance field, the block / cell split in front of the classes,
// and the accumulation of one (pose, point) pair into the eight counters of a pose's row — once, for the kernel
// (mlm_kernels_score.h), the host code (MapView::score, mlm_mapview.h) and the CPU test driver (tests/cpp/score_driver.cpp), so that
// all three run the very same arithmetic.  No reference counterpart: the reference takes its pose from an external odometry
// (mlmap.cpp:485-498) and never asks whether it agrees with the map; the classes of the voxels are those of its point queries (what
// mlm_export_window's occ / infl channels return), the field is mlm_export_esdf's sqdist.
//
// World position of point s under pose T = {R row major, o}: w_a = ((R[a][0] * s0 + R[a][1] * s1) + R[a][2] * s2) + o[a], five IEEE
// double operations per axis in that order, nothing fused (the library and the driver are built with -ffp-contract=off).  Lattice:
// Q_a = floor((w_a / d) * 1024.0), mlm_ray_lattice of mlm_raywalk.h; the pair is invalid if a Q is not finite or |Q| >= 2^40 and then
// touches no counter.  Voxel v = Q >> 10, so -2^30 <= v < 2^30 and v minus the first voxel of any block fits an int32.
//
// The classes come from a callable in the shape of mlm_raywalk.h's: `int cls(const int g[3], const int c[3], bool new_block)`, block
// index and cell coordinate of the voxel (v = g * n + c), new_block when g differs from the previous call's — the callee keeps the
// block's slot until then, so consecutive points inside one block cost one table probe together.  It returns the MLM_RAY_* bits:
// 1 getOccupancy == OCCUPIED, 2 getInflateOccupancy == OCCUPIED, 4 getOccupancy == UNKNOWN (neither 1 nor 4: FREE).
//
// Every counter is a count or a sum of integers <= 2^20 over at most 2^22 points: below 2^43, one value whatever the order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mlm_raywalk.h"

#define MLM_SCORE_WORDS 8            // MLM_SCORE_ROW of the header
#define MLM_SCORE_MAX_COUNT (1 << 22) // most points, most poses of a call
#define MLM_SCORE_MAX_CAP (1 << 20)   // largest sq_cap

// the distance field of a call: one int32 per voxel of the box lo <= v < lo + dims, [dims[2]][dims[1]][dims[0]]; sqdist null: none
struct MlmScoreField {
    const int32_t *sqdist;
    int32_t lo[3], dims[3];
    int32_t cap;
};

// the block the previous valid pair of this pose fell into: its index and its first voxel per axis
struct MlmScoreBlock {
    int g[3], base[3];
    bool have;
};

// a callable for calls without classes
struct MlmScoreNoClasses {
    MLM_RW_HD int operator()(const int *, const int *, bool) const { return 0; }
};

MLM_RW_HD void mlm_score_world(const double T[12], const double s[3], double w[3]) {
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) w[a] = ((T[3 * a] * s[0] + T[3 * a + 1] * s[1]) + T[3 * a + 2] * s[2]) + T[9 + a];
}

// the voxel of a world position; false: an invalid pair
MLM_RW_HD bool mlm_score_voxel(const double w[3], double d, int32_t v[3]) {
    bool ok = true;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        long long q = 0;
        ok = mlm_ray_lattice(w[a], d, q) && ok;
        v[a] = (int32_t)(q >> 10);
    }
    return ok;
}

// whether v lies in the field's box, and then its index there (below 2^31: mlm_box_check)
MLM_RW_HD bool mlm_score_in_box(const MlmScoreField &F, const int32_t v[3], size_t &at) {
    // (constant indices, no loop over the axes: the field's box is kernel-argument data and has to stay in scalar registers)
    const long long rx = (long long)v[0] - F.lo[0], ry = (long long)v[1] - F.lo[1], rz = (long long)v[2] - F.lo[2];
    const bool in = rx >= 0 && rx < F.dims[0] && ry >= 0 && ry < F.dims[1] && rz >= 0 && rz < F.dims[2];
    at = in ? (size_t)((rz * F.dims[1] + ry) * F.dims[0] + rx) : 0;
    return in;
}

// min(max(s, 0), cap)
MLM_RW_HD int32_t mlm_score_cost(int32_t s, int32_t cap) { return s < 0 ? 0 : (s > cap ? cap : s); }

// block index and cell coordinate of v; true when the block differs from the previous pair's (B is updated)
MLM_RW_HD bool mlm_score_cell(const int32_t v[3], int n, MlmScoreBlock &B, int c[3]) {
    bool same = B.have;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        c[a] = v[a] - B.base[a]; // (no overflow: see above)
        same = same && c[a] >= 0 && c[a] < n;
    }
    if (same) return false;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        const int g = v[a] >= 0 ? v[a] / n : -((-v[a] + n - 1) / n);
        B.g[a] = g;
        B.base[a] = g * n;
        c[a] = v[a] - g * n;
    }
    B.have = true;
    return true;
}

// One pair into the eight counters of its pose.  n = subbox_n, d = subbox_d_xyz.
template <bool CLASSES, bool FIELD, class Cls>
MLM_RW_HD void mlm_score_pair(const double T[12], const double s[3], double d, int n, const MlmScoreField &F, Cls &cls, MlmScoreBlock &B,
                              unsigned long long acc[MLM_SCORE_WORDS]) {
    double w[3];
    mlm_score_world(T, s, w);
    int32_t v[3];
    if (!mlm_score_voxel(w, d, v)) return;
    acc[0] += 1;
    if (CLASSES) {
        int c[3];
        const bool nb = mlm_score_cell(v, n, B, c);
        const int bits = cls(B.g, c, nb);
        acc[1] += (unsigned long long)(bits & 1);
        acc[2] += (unsigned long long)((bits & 5) == 0);
        acc[3] += (unsigned long long)((bits >> 2) & 1);
        acc[4] += (unsigned long long)((bits >> 1) & 1);
    }
    if (FIELD) { // (one update per counter, no branch around them: the counters stay in registers)
        size_t at;
        const bool in = mlm_score_in_box(F, v, at);
        const int32_t sq = in ? F.sqdist[at] : 0;
        acc[5] += (unsigned long long)in;
        acc[6] += (unsigned long long)(in ? mlm_score_cost(sq, F.cap) : F.cap);
        acc[7] += (unsigned long long)(in && sq <= 0);
    }
}
