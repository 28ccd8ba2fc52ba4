// mlm_reach.h — the per-voxel rules of mlm_export_reach (include/mlmap_hip.h): pure integer code shared by the kernels
// (mlm_kernels_reach.h) and the CPU test driver (tests/cpp/reach_driver.cpp), so that both run the very same arithmetic.  No
// reference counterpart: the reference has no cost-to-go field; the classes behind the traversable mask are those of its point
// queries (what mlm_export_window's occ / infl channels return), the field is defined here.
//
// The working field holds one u32 per voxel of the box: the steps found so far (the length of a real 6-connected path of
// traversable voxels from a seed, so never below the final value), MLM_REACH_FAR for a traversable voxel no path has reached yet,
// MLM_REACH_BLOCKED for a voxel that is not traversable — and for every voxel outside the box, which a path never enters.  The
// final field is the least fixpoint of steps(v) = min(steps(v), 1 + min over the six neighbours) with results above max_steps
// dropped; values only ever decrease towards it, so the order and grouping of relaxations do not matter.  That is the only
// property the tile schedule relies on:
//  - a seed stores 0 and marks its tile dirty — and, being a lowered voxel, the tile beyond every tile face it lies on;
//  - a tile (T[0] x T[1] x T[2] voxels, cut to the box) is relaxed to its own fixpoint against a one-voxel halo read from the field;
//  - a tile whose voxel on face c changed marks the tile beyond face c dirty for the NEXT sweep (that tile's halo is stale);
//  - a sweep relaxes the dirty tiles; the field is final when a sweep marks nothing.
// Every voxel whose shortest path crosses k tile faces is final after sweep k + 1 (induction over k: its predecessor beyond the last
// crossing became final in some sweep j <= k, whose tile marked this one for sweep j + 1), and one more sweep finds nothing to
// mark: at most min(max_steps, voxels - 1) + 2 sweeps (mlm_reach_plan's cap, mlm_host.h).
// Codes of faces, neighbours and parents: 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MLM_RE_HD __host__ __device__ __forceinline__
#else
#define MLM_RE_HD inline
#endif

#define MLM_REACH_BLOCKED 0xFFFFFFFFu // not traversable, or outside the box
#define MLM_REACH_FAR 0xFFFFFFFEu     // traversable, not reached (so far)

// one relaxation of a voxel from its six neighbours' values: the new value (== cur: nothing to store)
MLM_RE_HD uint32_t mlm_reach_relax(uint32_t cur, uint32_t xm, uint32_t xp, uint32_t ym, uint32_t yp, uint32_t zm, uint32_t zp,
                                   uint32_t max_steps) {
    if (cur == MLM_REACH_BLOCKED) return cur;
    uint32_t m = xm < xp ? xm : xp;
    const uint32_t my = ym < yp ? ym : yp, mz = zm < zp ? zm : zp;
    m = m < my ? m : my;
    m = m < mz ? m : mz;
    if (m >= MLM_REACH_FAR) return cur; // no neighbour reached
    const uint32_t cand = m + 1u;
    return (cand < cur && cand <= max_steps) ? cand : cur;
}

// the faces of a tile of td voxels that the tile's voxel (ix, iy, iz) lies on: bit c = face c
MLM_RE_HD unsigned mlm_reach_faces(int ix, int iy, int iz, const int td[3]) {
    return (ix == 0 ? 1u : 0u) | (ix == td[0] - 1 ? 2u : 0u) | (iy == 0 ? 4u : 0u) | (iy == td[1] - 1 ? 8u : 0u) | (iz == 0 ? 16u : 0u) |
           (iz == td[2] - 1 ? 32u : 0u);
}

// the tile beyond face c of tile (t0, t1, t2) in a grid of n tiles per axis: its linear index ([n2][n1][n0], x fastest), -1: none
MLM_RE_HD long long mlm_reach_tile_beyond(long long t0, long long t1, long long t2, const long long n[3], int c) {
    long long t[3] = {t0, t1, t2};
    const int a = c >> 1;
    t[a] += (c & 1) ? 1 : -1;
    if (t[a] < 0 || t[a] >= n[a]) return -1;
    return (t[2] * n[1] + t[1]) * n[0] + t[0];
}

// outputs of a voxel from its final value and its six neighbours' (MLM_REACH_BLOCKED beyond the box), in code order
MLM_RE_HD int32_t mlm_reach_steps(uint32_t v) { return v < MLM_REACH_FAR ? (int32_t)v : -1; }
MLM_RE_HD uint8_t mlm_reach_parent(uint32_t v, const uint32_t nb[6]) {
    if (v >= MLM_REACH_FAR) return 255;
    if (v == 0) return 6; // (MLM_REACH_SEED: only an effective seed has 0 steps)
    for (int c = 0; c < 6; ++c)
        if (nb[c] == v - 1u) return (uint8_t)c;
    return 255; // (not reached at the fixpoint: there v = 1 + the smallest neighbour)
}
