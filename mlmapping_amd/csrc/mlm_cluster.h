// mlm_cluster.h — the per-voxel rules of mlm_export_clusters (include/mlmap_hip.h): pure integer code shared by the kernels
// (mlm_kernels_cluster.h) and the CPU test driver (tests/cpp/cluster_driver.cpp), so that both run the very same arithmetic.  No
// reference counterpart: the reference has no clustering; the classes behind the set S are those of its point queries (what
// mlm_export_window's occ / infl channels return), components, numbering and statistics are defined here.
//
// The working field holds one u32 per voxel of the box: MLM_CLUSTER_OFF off S, else the linear box index of a voxel of the same
// component that is not larger than the voxel's own (a union-find parent; a root points at itself).  "Every voxel points at the
// smallest index of its component" is the least fixpoint of such fields under "take the smaller of what two joined voxels point
// at": entries only ever decrease, an entry never leaves its component, so the result does not depend on the order in which pairs
// are visited or on which of two racing writers wins.  The phases, each a launch (the launch boundary is the only ordering):
//  - local:   per tile, labels in tile-local order (z, y, x — which agrees with box order inside a tile, so a tile-local minimum
//             is the box minimum of the tile's piece): mlm_cluster_local_step on every voxel until a pass changes nothing;
//  - merge:   for every pair of S-neighbours that a tile face, edge or corner separates — each unordered pair once, from its
//             smaller voxel, through the forward offsets — mlm_cluster_union;
//  - flatten: every voxel of S points at its root (mlm_cluster_find), component sizes are counted at the roots;
//  - number:  kept roots (size >= min_size) get 0 .. K-1 in ascending index order; the root's size word becomes that number
//             (MLM_CLUSTER_OFF: dropped), and the root writes the start of its table row (mlm_cluster_row_init);
//  - write:   labels (mlm_cluster_label) and the rest of the rows (mlm_cluster_row_update: sums by addition, bounds by min / max,
//             face bits by or — order independent, hence exact).
// Codes of box faces: 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z (those of mlm_reach.h).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MLM_CL_HD __host__ __device__ __forceinline__
#else
#define MLM_CL_HD inline
#endif

#define MLM_CLUSTER_OFF 0xFFFFFFFFu // not in S (field); a dropped component (number word)
#define MLM_CLUSTER_ROW_I64 16      // (MLM_CLUSTER_ROW of the public header)

// the forward half of the neighbour offsets (dx, dy, dz): those that raise the linear index, by the number of non-zero entries;
// the other half are their negatives.  Connectivity 6 / 18 / 26 takes the first 3 / 9 / 13 (0: no such connectivity).
MLM_CL_HD int mlm_cluster_nfwd(int connectivity) { return connectivity == 6 ? 3 : connectivity == 18 ? 9 : connectivity == 26 ? 13 : 0; }
MLM_CL_HD void mlm_cluster_fwd(int k, int &dx, int &dy, int &dz) {
    // 2 bits per entry (0: -1, 1: 0, 2: +1), x | y << 2 | z << 4
    const unsigned char code[13] = {0x16, 0x19, 0x25, 0x1A, 0x18, 0x26, 0x24, 0x29, 0x21, 0x2A, 0x28, 0x22, 0x20};
    const int c = code[k];
    dx = (c & 3) - 1;
    dy = ((c >> 2) & 3) - 1;
    dz = (c >> 4) - 1;
}

// the root of v: ld(i) reads entry i of the field (entries on the way are members of v's component, each below the one before)
template <class Ld> MLM_CL_HD uint32_t mlm_cluster_find(Ld ld, uint32_t v) {
    for (uint32_t p = ld(v); p < v; p = ld(v)) v = p;
    return v;
}

// join the components of a and b: the larger root is linked under the smaller by amin(i, val) = atomic min on entry i that
// returns the entry's earlier value.  An earlier value other than the root itself means that another union linked it first: the
// entry now holds the smaller of the two links, and what it held before still has to be joined with b — from there again.
// Returns the number of atomics issued.
template <class Ld, class Amin> MLM_CL_HD unsigned mlm_cluster_union(Ld ld, Amin amin, uint32_t a, uint32_t b) {
    unsigned tries = 0;
    for (;;) {
        a = mlm_cluster_find(ld, a);
        b = mlm_cluster_find(ld, b);
        if (a == b) return tries;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        ++tries;
        const uint32_t old = amin(a, b);
        if (old == a) return tries;
        a = old;
    }
}

// one local step of the tile voxel (ix, iy, iz) of a tile of td voxels on the tile's labels s ([td2][td1][td0]: tile-local index
// of a voxel of the same component that is not larger, MLM_CLUSTER_OFF off S): the smallest label among itself and its
// S-neighbours inside the tile, followed to its root.  (== s[own]: nothing to store.  Other voxels may be stored meanwhile: any
// value read is a member of the component.)
MLM_CL_HD uint32_t mlm_cluster_local_step(const volatile uint32_t *s, int ix, int iy, int iz, const int td[3], int nfwd) {
    uint32_t m = s[(iz * td[1] + iy) * td[0] + ix];
    if (m == MLM_CLUSTER_OFF) return m;
    for (int k = 0; k < nfwd; ++k) {
        int dx, dy, dz;
        mlm_cluster_fwd(k, dx, dy, dz);
        for (int sg = 0; sg < 2; ++sg, dx = -dx, dy = -dy, dz = -dz) {
            const int x = ix + dx, y = iy + dy, z = iz + dz;
            if (x < 0 || x >= td[0] || y < 0 || y >= td[1] || z < 0 || z >= td[2]) continue;
            const uint32_t u = s[(z * td[1] + y) * td[0] + x];
            if (u < m) m = u; // (MLM_CLUSTER_OFF is the largest value)
        }
    }
    for (uint32_t p = s[m]; p < m; p = s[m]) m = p;
    return m;
}

// does the step (dx, dy, dz) from tile voxel (ix, iy, iz) leave the tile?
MLM_CL_HD bool mlm_cluster_leaves(int ix, int iy, int iz, int dx, int dy, int dz, const int td[3]) {
    const int x = ix + dx, y = iy + dy, z = iz + dz;
    return x < 0 || x >= td[0] || y < 0 || y >= td[1] || z < 0 || z >= td[2];
}

// the faces of the box of D voxels that box voxel (x, y, z) lies on: bit c = face c
MLM_CL_HD unsigned mlm_cluster_faces(long long x, long long y, long long z, const long long D[3]) {
    return (x == 0 ? 1u : 0u) | (x == D[0] - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == D[1] - 1 ? 8u : 0u) | (z == 0 ? 16u : 0u) |
           (z == D[2] - 1 ? 32u : 0u);
}

// the label of a voxel from its field entry (its root after flatten) and the number word of that root
MLM_CL_HD int32_t mlm_cluster_label(uint32_t root, uint32_t number_of_root) {
    if (root == MLM_CLUSTER_OFF) return -1;                       // MLM_CLUSTER_NONE
    return number_of_root == MLM_CLUSTER_OFF ? -2 : (int32_t)number_of_root; // MLM_CLUSTER_SMALL
}

// a kept component's table row as its root starts it: size, the root (box voxel r[], box origin lo[]), bounds that hold the root
MLM_CL_HD void mlm_cluster_row_init(int64_t *row, uint32_t size, const long long r[3], const long long lo[3]) {
    row[0] = size;
    for (int a = 0; a < 3; ++a) {
        row[1 + a] = row[4 + a] = row[7 + a] = lo[a] + r[a];
        row[10 + a] = 0;
    }
    row[13] = row[14] = row[15] = 0;
}
// ... and what voxels of the component add (mn / mx: smallest / largest box coordinates of some of them, sum: their sum, faces:
// the or of their face bits) through add / amin / amax / aor on an int64 (each may skip a value that cannot change the entry)
template <class Add, class Min, class Max, class Or>
MLM_CL_HD void mlm_cluster_row_update(int64_t *row, const long long mn[3], const long long mx[3], const long long sum[3], unsigned faces,
                                      const long long lo[3], Add add, Min amin, Max amax, Or aor) {
    for (int a = 0; a < 3; ++a) {
        amin(&row[4 + a], (int64_t)(lo[a] + mn[a]));
        amax(&row[7 + a], (int64_t)(lo[a] + mx[a]));
        add(&row[10 + a], (int64_t)sum[a]);
    }
    if (faces) aor(&row[13], (int64_t)faces);
}
