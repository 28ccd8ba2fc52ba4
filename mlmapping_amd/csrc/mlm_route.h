// mlm_route.h — the per-voxel rules of mlm_export_route (include/mlmap_hip.h): pure integer code shared by the kernels
// (mlm_kernels_route.h) and the CPU test driver (tests/cpp/route_driver.cpp), so that both run the very same arithmetic.  No
// reference counterpart: the reference has no cost field; the classes behind the traversable mask are those of its point queries,
// the distance behind the rings is mlm_export_esdf's D_out, the field is defined here.
//
// The working field is mlm_reach.h's: one u32 per voxel of the box, the cost of a real path of permitted moves from a seed (so
// never below the final value), MLM_REACH_FAR for a traversable voxel no path has reached yet, MLM_REACH_BLOCKED for a voxel that
// is not traversable and for every voxel outside the box.  The final field is the least fixpoint of
// cost(v) = min(cost(v), cost(u) + move_cost + pen(v)) over the permitted moves u -> v, with results above max_cost dropped.  All
// edge weights are positive integers, values only ever decrease towards the fixpoint, so the order and grouping of relaxations do
// not matter, and the tile schedule of mlm_reach.h carries over: a tile is relaxed to its own fixpoint against a one-voxel halo
// (edges and corners of the halo box included: a diagonal move reads them), a lowered voxel marks every neighbouring tile whose
// halo holds it, a sweep relaxes the marked tiles, the field is final when a sweep marks nothing.  A voxel whose optimal path
// crosses k tile boundaries is final after sweep k + 1 (the induction of mlm_reach.h; the path has at most voxels - 1 moves),
// hence mlm_route_plan's cap of voxels + 1 sweeps (mlm_host.h).
// A stored value is at most max_cost <= 2^31 - 1 and a candidate adds at most 65535 + 65535, so u32 never wraps.
//
// Offsets and parent codes (dx, dy, dz): 0..5 the faces -x, +x, -y, +y, -z, +z (mlm_reach.h's); 6..17 the offsets with two non-zero
// entries and 18..25 the corners, each group in ascending order of (dz, dy, dx).  Connectivity 6 / 18 / 26 takes the first 6 / 18 /
// 26.  The move u -> v = u + o is permitted iff u, v and every u + o' are traversable, o' being o with a non-empty proper subset
// of its non-zero entries zeroed: seen from v, every voxel v + q with q a non-zero sub-offset of -o (-o itself included) — the
// same set, so the rule is symmetric and is tested on v's own 3 x 3 x 3 neighbourhood.
#pragma once
#include <stdint.h>

#include "mlm_reach.h"

#define MLM_ROUTE_CODES 26
#ifdef __HIPCC__
#define MLM_ROUTE_UNROLL _Pragma("unroll")
#else
#define MLM_ROUTE_UNROLL
#endif
#define MLM_ROUTE_CLASS_BLOCKED 255 // class byte of a voxel that is not traversable

// offset of code c
MLM_RE_HD void mlm_route_offset(int c, int &dx, int &dy, int &dz) {
    // 2 bits per entry (0: -1, 1: 0, 2: +1), x | y << 2 | z << 4
    const unsigned char code[MLM_ROUTE_CODES] = {0x14, 0x16, 0x11, 0x19, 0x05, 0x25, 0x01, 0x04, 0x06, 0x09, 0x10, 0x12, 0x18,
                                                 0x1A, 0x21, 0x24, 0x26, 0x29, 0x00, 0x02, 0x08, 0x0A, 0x20, 0x22, 0x28, 0x2A};
    const int k = code[c];
    dx = (k & 3) - 1;
    dy = ((k >> 2) & 3) - 1;
    dz = (k >> 4) - 1;
}
// index into move_cost of code c: non-zero entries - 1
MLM_RE_HD int mlm_route_kind(int c) { return c < 6 ? 0 : c < 18 ? 1 : 2; }
MLM_RE_HD bool mlm_route_connectivity_ok(int connectivity) { return connectivity == 6 || connectivity == 18 || connectivity == 26; }

// is the move between v and v + (dx, dy, dz) permitted, v itself being traversable?  at(x, y, z): the working value of the voxel
// v + (x, y, z), MLM_REACH_BLOCKED outside the box
template <class At> MLM_RE_HD bool mlm_route_permitted(At at, int dx, int dy, int dz) {
    const int nz = (dx ? 1 : 0) | (dy ? 2 : 0) | (dz ? 4 : 0);
    for (int k = 1; k < 8; ++k) {
        if ((k & nz) != k) continue;
        if (at((k & 1) ? dx : 0, (k & 2) ? dy : 0, (k & 4) ? dz : 0) == MLM_REACH_BLOCKED) return false;
    }
    return true;
}

// one relaxation of a voxel with value cur and entry penalty pen from its neighbours of the first CONN codes: the new value
// (== cur: nothing to store)
template <int CONN, class At> MLM_RE_HD uint32_t mlm_route_relax(uint32_t cur, uint32_t pen, const uint32_t move_cost[3], uint32_t max_cost, At at) {
    if (cur == MLM_REACH_BLOCKED) return cur;
    uint32_t best = cur;
    MLM_ROUTE_UNROLL
    for (int c = 0; c < CONN; ++c) {
        int dx, dy, dz;
        mlm_route_offset(c, dx, dy, dz);
        if (!mlm_route_permitted(at, dx, dy, dz)) continue;
        const uint32_t u = at(dx, dy, dz);
        if (u >= MLM_REACH_FAR) continue;
        const uint32_t cand = u + move_cost[mlm_route_kind(c)] + pen;
        if (cand < best && cand <= max_cost) best = cand;
    }
    return best;
}

// outputs of a voxel from its final value, its entry penalty and its neighbourhood's final values
MLM_RE_HD int32_t mlm_route_cost(uint32_t v) { return v < MLM_REACH_FAR ? (int32_t)v : -1; }
template <class At> MLM_RE_HD uint8_t mlm_route_parent(uint32_t v, uint32_t pen, const uint32_t move_cost[3], int connectivity, At at) {
    if (v >= MLM_REACH_FAR) return 255;
    if (v == 0) return MLM_ROUTE_CODES; // (MLM_ROUTE_SEED: every move costs 1 at least, so only an effective seed has cost 0)
    for (int c = 0; c < connectivity; ++c) {
        int dx, dy, dz;
        mlm_route_offset(c, dx, dy, dz);
        if (!mlm_route_permitted(at, dx, dy, dz)) continue;
        const uint32_t u = at(dx, dy, dz);
        if (u < MLM_REACH_FAR && u + move_cost[mlm_route_kind(c)] + pen == v) return (uint8_t)c;
    }
    return 255; // (not reached at the fixpoint)
}

// class byte of a voxel from its D_out (mlm_export_esdf's, truncated at (r + n_penalty + 1)^2): MLM_ROUTE_CLASS_BLOCKED if
// D_out <= r^2, else min(k, n_penalty) for the smallest k with D_out <= (r + 1 + k)^2 — its ring
MLM_RE_HD uint8_t mlm_route_class(unsigned d_out, int r, int n_penalty) {
    if (d_out <= (unsigned)(r * r)) return MLM_ROUTE_CLASS_BLOCKED;
    int k = 0;
    while (k < n_penalty && d_out > (unsigned)((r + 1 + k) * (r + 1 + k))) ++k;
    return (uint8_t)k;
}
// entry penalty of a class byte from the table of 64 words (penalty[0 .. n_penalty - 1], then zeros); blocked voxels, whose
// penalty nobody uses, read word 63 (n_penalty <= 63: a zero)
MLM_RE_HD uint32_t mlm_route_pen(const uint32_t *table, uint8_t cls) { return table[cls & 63]; }

// the neighbouring tiles whose halo holds a voxel that lies on the tile faces `faces` (mlm_reach_faces): bit
// (tz + 1) * 9 + (ty + 1) * 3 + tx + 1 for the tile offset (tx, ty, tz) — every non-zero offset whose non-zero entries each point
// through a face the voxel lies on, with as many non-zero entries as the connectivity's moves have (6: the face tiles, 18: the
// edge tiles too, 26: the corner tiles too)
MLM_RE_HD uint32_t mlm_route_dirty_mask(unsigned faces, int connectivity) {
    const int most = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    uint32_t m = 0;
    for (int i = 0; i < 27; ++i) {
        if (i == 13) continue;
        const int t[3] = {i % 3 - 1, (i / 3) % 3 - 1, i / 9 - 1};
        int nnz = 0;
        bool on = true;
        for (int a = 0; a < 3; ++a) {
            if (!t[a]) continue;
            ++nnz;
            on = on && ((faces >> (2 * a + (t[a] > 0 ? 1 : 0))) & 1u);
        }
        if (on && nnz <= most) m |= 1u << i;
    }
    return m;
}
// the tile at offset bit i of mlm_route_dirty_mask from tile (t0, t1, t2) in a grid of n tiles per axis: its linear index, -1: none
MLM_RE_HD long long mlm_route_tile_at(long long t0, long long t1, long long t2, const long long n[3], int i) {
    const long long t[3] = {t0 + i % 3 - 1, t1 + (i / 3) % 3 - 1, t2 + i / 9 - 1};
    for (int a = 0; a < 3; ++a)
        if (t[a] < 0 || t[a] >= n[a]) return -1;
    return (t[2] * n[1] + t[1]) * n[0] + t[0];
}
