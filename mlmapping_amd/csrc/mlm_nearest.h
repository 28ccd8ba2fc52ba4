// mlm_nearest.h — the nearest obstacle voxel of mlm_query_nearest (include/mlmap_hip.h): the lattice step, the metric, the packed key
// whose unsigned minimum is the contract's tie rule, the bounds and the ring search, once, for the kernel (mlm_kernels_nearest.h), the
// host mirror (MapView::nearest, mlm_mapview.h) and the CPU test driver (tests/cpp/nearest_driver.cpp), so that all three run the very
// same control flow.  No reference counterpart: the reference has no nearest-obstacle query; the classes of the voxels are those of its
// point queries (what mlm_export_window's occ / infl channels return).
//
// A point is Q[3] (mlm_ray_lattice of mlm_raywalk.h: 1024 lattice units per voxel), kept as its voxel v = Q >> 10 and the remainder
// r = Q & 1023.  The vector from the point to the centre of voxel o is delta_a = 1024 * (o_a - v_a) + 512 - r_a: with |o_a - v_a| <= 64
// it fits 18 bits, its square 35, E = sum of the squares stays below 2^34 for the candidates (E <= (1024 * C)^2 = 2^32 at C = 64).
//
// The answer is the BRUTE-FORCE minimum of the key over every voxel of the map with O and E <= (1024 * C)^2; the pruning below is
// invisible: a block (a ring of blocks) is skipped only if a lower bound of E over it is STRICTLY greater than the smallest E found so
// far — a block with an equal bound may still hold a voxel that wins by the tie rule.
//
// The voxels come from a callable with two members, both run with wave-uniform arguments on the device:
//     int probe(const int g[3])
//         looks block g up and keeps it; returns -1 if the block has a class per voxel, else the MLM_NEAR_* bits that hold at EVERY
//         voxel of it (an absent block: UNKNOWN; a released block: what element 0 says, inflated class UNKNOWN);
//     unsigned long long scan(const MlmNearPoint &p, const int g[3], const int c0[3], const int c1[3], int flags)
//         the smallest mlm_near_voxel_key over the cells c0 .. c1 (inclusive, per axis) of the block last probed whose classes meet
//         flags, MLM_NEAR_NOKEY if there is none.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mlm_raywalk.h"

#define MLM_NEAR_MAX_DIST 64
#define MLM_NEAR_NOKEY 0xFFFFFFFFFFFFFFFFull

struct MlmNearPoint {
    int32_t v[3], r[3]; // voxel and remainder of Q per axis
    long long lim;      // (1024 * C)^2
    int C;
};

struct MlmNearResult {
    int status;        // 1 found, 0 nothing in range, -1 invalid point
    int32_t voxel[3];  // the obstacle voxel, or v
    int32_t delta[3];  // point -> its centre in 1/1024 voxel, or 0
    long long sq;      // E, or -1
    double dist;       // metres, or -1.0
};

// the lattice step; false: an invalid point
MLM_RW_HD bool mlm_near_point(const double pos[3], double d, int C, MlmNearPoint &p) {
    bool ok = true;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        long long q = 0;
        ok = mlm_ray_lattice(pos[a], d, q) && ok;
        p.v[a] = (int32_t)(q >> 10);
        p.r[a] = (int32_t)(q & 1023);
    }
    p.lim = (long long)(1024 * C) * (1024 * C);
    p.C = C;
    return ok;
}

MLM_RW_HD int32_t mlm_near_delta(const MlmNearPoint &p, int a, int32_t o) { return 1024 * (o - p.v[a]) + 512 - p.r[a]; }

MLM_RW_HD long long mlm_near_sq(const MlmNearPoint &p, const int32_t o[3]) {
    long long e = 0;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        const long long dl = mlm_near_delta(p, a, o[a]);
        e += dl * dl;
    }
    return e;
}

// E * 2^24 + (o_z - v_z + 64) * 2^16 + (o_y - v_y + 64) * 2^8 + (o_x - v_x + 64) of a voxel of the cube v +- C
MLM_RW_HD unsigned long long mlm_near_pack(const MlmNearPoint &p, long long e, const int32_t o[3]) {
    return ((unsigned long long)e << 24) | ((unsigned long long)(uint32_t)(o[2] - p.v[2] + 64) << 16) |
           ((unsigned long long)(uint32_t)(o[1] - p.v[1] + 64) << 8) | (unsigned long long)(uint32_t)(o[0] - p.v[0] + 64);
}

// the key of a voxel of the cube that has O: outside the ball it is no candidate
MLM_RW_HD unsigned long long mlm_near_voxel_key(const MlmNearPoint &p, const int32_t o[3]) {
    const long long e = mlm_near_sq(p, o);
    return e <= p.lim ? mlm_near_pack(p, e, o) : MLM_NEAR_NOKEY;
}

// The o in lo .. hi (lo <= hi) with the smallest |delta_a|, ties to the smaller o.  Without the range it is v, or v - 1 when the
// point lies on the face between the two (r == 0: both at 512); |delta_a| grows with the distance from there on either side.
MLM_RW_HD int32_t mlm_near_axis_best(const MlmNearPoint &p, int a, int32_t lo, int32_t hi) {
    const int32_t t = p.r[a] == 0 ? p.v[a] - 1 : p.v[a];
    return t < lo ? lo : (t > hi ? hi : t);
}

MLM_RW_HD int mlm_near_fdiv(int v, int n) { return v >= 0 ? v / n : -((-v + n - 1) / n); }

// A lower bound of E over every block of ring k >= 1 (Chebyshev distance k from v's block gv): such a block lies k blocks away on some
// axis, on one side; the squared distance along that axis alone to the nearest centre of that slab of blocks.  It grows with k.
MLM_RW_HD long long mlm_near_ring_bound(const MlmNearPoint &p, const int gv[3], int n, int k) {
    long long best = 0x7FFFFFFFFFFFFFFFll;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        const long long up = mlm_near_delta(p, a, (gv[a] + k) * n);            // > 0: the first voxel of the slab above
        const long long dn = -(long long)mlm_near_delta(p, a, (gv[a] - k) * n + n - 1); // > 0: the last voxel of the slab below
        const long long m = up < dn ? up : dn;
        best = m * m < best ? m * m : best;
    }
    return best;
}

MLM_RW_HD void mlm_near_none(const MlmNearPoint &p, bool valid, MlmNearResult &o) {
    o.status = valid ? 0 : -1;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        o.voxel[a] = valid ? p.v[a] : 0;
        o.delta[a] = 0;
    }
    o.sq = -1;
    o.dist = -1.0;
}

// The ring search for a point already on the lattice: the smallest key, or MLM_NEAR_NOKEY.  n = subbox_n.  (Also the full ball at the
// start voxel of mlm_query_sweeps: mlm_sweep.h.)
template <class Vox> MLM_RW_HD unsigned long long mlm_near_best(const MlmNearPoint &p, int n, int flags, Vox &vox) {
    const int C = p.C;
    int gv[3], g0[3], g1[3], K = 0;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        gv[a] = mlm_near_fdiv(p.v[a], n);
        g0[a] = mlm_near_fdiv(p.v[a] - C, n);
        g1[a] = mlm_near_fdiv(p.v[a] + C, n);
        K = gv[a] - g0[a] > K ? gv[a] - g0[a] : K;
        K = g1[a] - gv[a] > K ? g1[a] - gv[a] : K;
    }
    unsigned long long best = MLM_NEAR_NOKEY;
    long long cut = p.lim; // the smallest E so far, or the ball
    for (int k = 0; k <= K; ++k) {
        if (k > 0 && mlm_near_ring_bound(p, gv, n, k) > cut) break;
        const int zl = gv[2] - k > g0[2] ? gv[2] - k : g0[2], zh = gv[2] + k < g1[2] ? gv[2] + k : g1[2];
        const int yl = gv[1] - k > g0[1] ? gv[1] - k : g0[1], yh = gv[1] + k < g1[1] ? gv[1] + k : g1[1];
        const int xl = gv[0] - k > g0[0] ? gv[0] - k : g0[0], xh = gv[0] + k < g1[0] ? gv[0] + k : g1[0];
        for (int gz = zl; gz <= zh; ++gz)
            for (int gy = yl; gy <= yh; ++gy) {
                const bool shell = gz - gv[2] == k || gv[2] - gz == k || gy - gv[1] == k || gv[1] - gy == k;
                for (int gx = xl; gx <= xh; ++gx) {
                    if (!shell && gx > gv[0] - k && gx < gv[0] + k) { // inside the ring: on to its far side
                        gx = gv[0] + k - 1;
                        continue;
                    }
                    const int g[3] = {gx, gy, gz};
                    // the part of the block inside the cube, and per axis its voxel nearest to the point: the bound, reached there
                    int c0[3], c1[3];
                    int32_t ob[3];
                    MLM_RW_UNROLL
                    for (int a = 0; a < 3; ++a) {
                        const int32_t b0 = g[a] * n, lo = b0 > p.v[a] - C ? b0 : p.v[a] - C, hi = b0 + n - 1 < p.v[a] + C ? b0 + n - 1 : p.v[a] + C;
                        c0[a] = lo - b0;
                        c1[a] = hi - b0;
                        ob[a] = mlm_near_axis_best(p, a, lo, hi);
                    }
                    const long long bound = mlm_near_sq(p, ob);
                    if (bound > cut) continue;
                    const int whole = vox.probe(g);
                    unsigned long long key;
                    if (whole >= 0) {
                        if (!(whole & flags)) continue;
                        key = mlm_near_pack(p, bound, ob); // (E is a sum over the axes and the tie order lexicographic: the block's smallest key)
                    } else {
                        key = vox.scan(p, g, c0, c1, flags);
                    }
                    if (key < best) {
                        best = key;
                        cut = (long long)(key >> 24);
                    }
                }
            }
    }
    return best;
}

// The whole contract for one point.  n = subbox_n, d = subbox_d_xyz.
template <class Vox> MLM_RW_HD void mlm_near_search(const double pos[3], double d, int n, int C, int flags, Vox &vox, MlmNearResult &o) {
    MlmNearPoint p;
    if (!mlm_near_point(pos, d, C, p)) {
        mlm_near_none(p, false, o);
        return;
    }
    const unsigned long long best = mlm_near_best(p, n, flags, vox);
    if (best == MLM_NEAR_NOKEY) {
        mlm_near_none(p, true, o);
        return;
    }
    o.status = 1;
    o.voxel[0] = p.v[0] + (int32_t)(best & 255u) - 64;
    o.voxel[1] = p.v[1] + (int32_t)((best >> 8) & 255u) - 64;
    o.voxel[2] = p.v[2] + (int32_t)((best >> 16) & 255u) - 64;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) o.delta[a] = mlm_near_delta(p, a, o.voxel[a]);
    o.sq = (long long)(best >> 24);
    o.dist = ((double)(float)d * sqrt((double)o.sq)) / 1024.0; // (three IEEE operations; nothing to fuse)
}
