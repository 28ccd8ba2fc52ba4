// mlm_octree.h — the rules of mlm_export_octree (include/mlmap_hip.h): pure integer code shared by the kernels
// (mlm_kernels_octree.h) and the CPU test driver (tests/cpp/octree_driver.cpp), so that both run the very same arithmetic.  No
// reference counterpart: the reference publishes point markers; the classes behind the labels are those of its point queries (what
// mlm_export_window's occ / infl channels return), the tree and its numbering are defined here.
//
// Keys and cells: a voxel index v has the key k = v + 2^(depth - 1) per axis, 0 <= k < 2^depth; the level-l cell of a key is k >> l.
// A brick is a level-T cell, T = min(depth, 4): 16^3 voxels (the whole key cube below depth 4).  The working arrays of a call:
//  - the pyramid of one brick (MlmOctBrick: LDS on the device, a local on the host): labels of levels 0..T, per cell of levels 1..T
//    the inner nodes and the leaves of its subtree, and — on the way down — the numbers of its first inner node and first leaf;
//  - the upper arrays (MlmOctUpper, device memory): the same five values per cell of levels T..depth, level by level, each level the
//    cells that meet the box ([n2][n1][n0] from the level's lowest cell); level T are the bricks.
// Up: a cell's label, inner count and leaf count from its eight children (mlm_oct_reduce).  Down: an inner cell hands each child the
// numbers its subtree starts at, an exclusive prefix over the children in order (mlm_oct_hand_down), and writes its own row and the
// rows of its leaf children.  The numbering is that prefix and nothing else: no order of arrival enters it.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifdef __HIPCC__
#define MLM_OCT_HD __host__ __device__ __forceinline__
#else
#define MLM_OCT_HD inline
#endif

#define MLM_OCT_F_INFL 1     // (MLM_OCT_INFL of the public header)
#define MLM_OCT_F_OCC_ONLY 2 // (MLM_OCT_OCC_ONLY)
#define MLM_OCT_ROW_I64 40   // (MLM_OCT_ROW)

// labels of a cell, the two bits a word holds per child
#define MLM_OCT_NONE 0
#define MLM_OCT_FREE 1
#define MLM_OCT_OCC 2
#define MLM_OCT_INNER 3

constexpr int kOctBrickLevel = 4;                         // a brick is 16^3 voxels
constexpr int kOctBrickCells = 4096 + 512 + 64 + 8 + 1;   // cells of levels 0..4
constexpr int kOctBrickUpper = 512 + 64 + 8 + 1;          // ... of levels 1..4
constexpr long long kOctCtrlBytes = 1024;
// the control block (u64 each): leaves per level, OCC then FREE, voxels per class, and what the root says
constexpr int kOctCtrlOccLeaves = 0, kOctCtrlFreeLeaves = 32, kOctCtrlOccVox = 64, kOctCtrlFreeVox = 65, kOctCtrlN = 66, kOctCtrlM = 67,
              kOctCtrlRoot = 68, kOctCtrlWords = 69;
constexpr long long kOctStageRows = 1ll << 20; // rows of a range staged for host destinations (22 B per inner node, 17 B per leaf)

// the label of a voxel from its classes (occ: 0 OCCUPIED, 1 FREE, -1 UNKNOWN; infl: 0 OCCUPIED, else -1) and the flags; a voxel outside
// the box is MLM_OCT_NONE without a look at the map
MLM_OCT_HD int mlm_oct_class(int occ, int infl, int flags) {
    if (occ == 0 || ((flags & MLM_OCT_F_INFL) && infl == 0)) return MLM_OCT_OCC;
    return occ == 1 && !(flags & MLM_OCT_F_OCC_ONLY) ? MLM_OCT_FREE : MLM_OCT_NONE;
}
// leaf_class of a leaf's label: the project's enum, 0 OCCUPIED, 1 FREE
MLM_OCT_HD int8_t mlm_oct_leaf_class(int label) { return (int8_t)(label == MLM_OCT_OCC ? 0 : 1); }

// child i of a cell: bit 0 from x, bit 1 from y, bit 2 from z of the next key bit
MLM_OCT_HD int mlm_oct_child_x(int i) { return i & 1; }
MLM_OCT_HD int mlm_oct_child_y(int i) { return (i >> 1) & 1; }
MLM_OCT_HD int mlm_oct_child_z(int i) { return i >> 2; }

// A cell from its eight children in order: the word, the label (NONE: all NONE; a leaf: all eight the same leaf; INNER otherwise),
// and the inner nodes and leaves of its subtree (an inner cell counts itself, a leaf is one leaf).  A voxel is a child with no inner
// node and one leaf unless it is NONE.
struct MlmOctNode {
    unsigned word;
    int label, inner, leaves;
};
MLM_OCT_HD MlmOctNode mlm_oct_reduce(const int lab[8], const int inner[8], const int leaves[8]) {
    MlmOctNode r{0u, MLM_OCT_NONE, 0, 0};
    int ni = 0, nl = 0;
    for (int i = 0; i < 8; ++i) {
        r.word |= (unsigned)lab[i] << (2 * i);
        ni += inner[i];
        nl += leaves[i];
    }
    if (r.word == 0u) return r;
    if (r.word == 0xAAAAu || r.word == 0x5555u) {
        r.label = r.word == 0xAAAAu ? MLM_OCT_OCC : MLM_OCT_FREE;
        r.leaves = 1;
        return r;
    }
    r.label = MLM_OCT_INNER;
    r.inner = 1 + ni;
    r.leaves = nl;
    return r;
}
// Down: inner node number ib with first leaf lb hands child i the numbers its subtree starts at — pre-order, children in order
MLM_OCT_HD void mlm_oct_hand_down(int ib, int lb, const int inner[8], const int leaves[8], int cib[8], int clb[8]) {
    int ri = ib + 1, rl = lb;
    for (int i = 0; i < 8; ++i) {
        cib[i] = ri;
        clb[i] = rl;
        ri += inner[i];
        rl += leaves[i];
    }
}

// Geometry of a call, built once on the host (mlm_oct_geo)
struct MlmOctGeo {
    long long lo[3], D[3];    // the box
    long long klo[3], khi[3]; // its keys, [klo, khi)
    long long half;           // 2^(depth - 1)
    long long off[33];        // upper arrays: the first cell of level l, l = T..depth; off[depth + 1]: all cells
    int depth, T, flags;
};
// the cells of level l that meet the box: the lowest per axis, and how many
MLM_OCT_HD long long mlm_oct_cell_lo(const MlmOctGeo &G, int l, int a) { return G.klo[a] >> l; }
MLM_OCT_HD long long mlm_oct_cell_n(const MlmOctGeo &G, int l, int a) { return ((G.khi[a] - 1) >> l) - (G.klo[a] >> l) + 1; }
// cell j of level l (counted within the level) -> its absolute cell coordinates; a level has fewer than 2^32 cells
MLM_OCT_HD void mlm_oct_cell_at(const MlmOctGeo &G, int l, long long j, long long c[3]) {
    const uint32_t n0 = (uint32_t)mlm_oct_cell_n(G, l, 0), n1 = (uint32_t)mlm_oct_cell_n(G, l, 1);
    const uint32_t row = (uint32_t)j / n0, z = row / n1;
    c[0] = mlm_oct_cell_lo(G, l, 0) + ((uint32_t)j - row * n0);
    c[1] = mlm_oct_cell_lo(G, l, 1) + (row - z * n1);
    c[2] = mlm_oct_cell_lo(G, l, 2) + z;
}
// ... and back: the index into the upper arrays of the level-l cell c, -1 if it does not meet the box
MLM_OCT_HD long long mlm_oct_cell_index(const MlmOctGeo &G, int l, const long long c[3]) {
    long long r[3];
    for (int a = 0; a < 3; ++a) {
        r[a] = c[a] - mlm_oct_cell_lo(G, l, a);
        if (r[a] < 0 || r[a] >= mlm_oct_cell_n(G, l, a)) return -1;
    }
    return G.off[l] + (r[2] * mlm_oct_cell_n(G, l, 1) + r[1]) * mlm_oct_cell_n(G, l, 0) + r[0];
}

// The rows the caller asked for: the inner nodes numbered [n0, n1) and the leaves numbered [m0, m1); the arrays point at row n0 / m0,
// each may be null
struct MlmOctOut {
    uint16_t *words;
    int32_t *inner4, *skip;
    long long n0, n1;
    int32_t *leaf4;
    int8_t *leaf_class;
    long long m0, m1;
};
// inner node n: the cell with lower corner key kx, ky, kz at `level`, `inner` inner nodes in its subtree (itself included)
MLM_OCT_HD void mlm_oct_inner_row(const MlmOctGeo &G, const MlmOctOut &O, long long n, unsigned word, long long kx, long long ky, long long kz,
                                  int level, int inner) {
    if (n < O.n0 || n >= O.n1) return;
    const size_t r = (size_t)(n - O.n0);
    if (O.words) O.words[r] = (uint16_t)word;
    if (O.inner4) {
        O.inner4[4 * r] = (int32_t)(kx - G.half);
        O.inner4[4 * r + 1] = (int32_t)(ky - G.half);
        O.inner4[4 * r + 2] = (int32_t)(kz - G.half);
        O.inner4[4 * r + 3] = level;
    }
    if (O.skip) O.skip[r] = (int32_t)(n + inner);
}
MLM_OCT_HD void mlm_oct_leaf_row(const MlmOctGeo &G, const MlmOctOut &O, long long m, long long kx, long long ky, long long kz, int level, int label) {
    if (m < O.m0 || m >= O.m1) return;
    const size_t r = (size_t)(m - O.m0);
    if (O.leaf4) {
        O.leaf4[4 * r] = (int32_t)(kx - G.half);
        O.leaf4[4 * r + 1] = (int32_t)(ky - G.half);
        O.leaf4[4 * r + 2] = (int32_t)(kz - G.half);
        O.leaf4[4 * r + 3] = level;
    }
    if (O.leaf_class) O.leaf_class[r] = mlm_oct_leaf_class(label);
}

// a counter of the control block: every lane may add (the counters are sums, no number depends on them)
MLM_OCT_HD void mlm_oct_count(unsigned long long *p, unsigned long long v) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// ---- one brick -------------------------------------------------------------------------------------------------------------------
// Level l of a brick is [s][s][s] cells, s = 2^(T - l), x fastest.  The levels lie at fixed places whatever T is.
struct MlmOctBrick {
    uint8_t lab[kOctBrickCells];                      // labels of levels 0..T
    uint16_t icnt[kOctBrickUpper], lcnt[kOctBrickUpper]; // levels 1..T: inner nodes and leaves of the subtree
    int32_t ib[kOctBrickUpper], lb[kOctBrickUpper];   // levels 1..T: first inner node (the cell itself if INNER) and first leaf; -1: not in the tree
};
MLM_OCT_HD int mlm_oct_lab_at(int l) { return l == 0 ? 0 : l == 1 ? 4096 : l == 2 ? 4608 : l == 3 ? 4672 : 4680; }
MLM_OCT_HD int mlm_oct_cnt_at(int l) { return l == 1 ? 0 : l == 2 ? 512 : l == 3 ? 576 : 584; }
// cell j of level l -> the places of its eight children in level l - 1, and its own coordinates
MLM_OCT_HD void mlm_oct_brick_children(int T, int l, int j, int ci[8], int &x, int &y, int &z) {
    const int sh = T - l, s = 1 << sh;
    x = j & (s - 1);
    y = (j >> sh) & (s - 1);
    z = j >> (2 * sh);
    for (int i = 0; i < 8; ++i)
        ci[i] = ((2 * z + mlm_oct_child_z(i)) << (2 * (sh + 1))) + ((2 * y + mlm_oct_child_y(i)) << (sh + 1)) + 2 * x + mlm_oct_child_x(i);
}
// the children's labels, inner counts and leaf counts of a brick cell
MLM_OCT_HD void mlm_oct_brick_gather(const MlmOctBrick &B, int l, const int ci[8], int lab[8], int inner[8], int leaves[8]) {
    for (int i = 0; i < 8; ++i) {
        lab[i] = B.lab[mlm_oct_lab_at(l - 1) + ci[i]];
        inner[i] = l == 1 ? 0 : B.icnt[mlm_oct_cnt_at(l - 1) + ci[i]];
        leaves[i] = l == 1 ? (lab[i] != MLM_OCT_NONE ? 1 : 0) : B.lcnt[mlm_oct_cnt_at(l - 1) + ci[i]];
    }
}
// Up: cell j of level l (1..T) from level l - 1.  cnt (may be null) collects what the summary counts below the brick's top: [0..3] OCC
// leaves of levels 0..3 — a leaf child of an inner cell is a leaf of the tree —, [4..7] FREE leaves, [8] OCC voxels, [9] FREE voxels.
MLM_OCT_HD void mlm_oct_brick_up(MlmOctBrick &B, int T, int l, int j, unsigned *cnt) {
    int ci[8], x, y, z, lab[8], inner[8], leaves[8];
    mlm_oct_brick_children(T, l, j, ci, x, y, z);
    mlm_oct_brick_gather(B, l, ci, lab, inner, leaves);
    const MlmOctNode r = mlm_oct_reduce(lab, inner, leaves);
    B.lab[mlm_oct_lab_at(l) + j] = (uint8_t)r.label;
    B.icnt[mlm_oct_cnt_at(l) + j] = (uint16_t)r.inner;
    B.lcnt[mlm_oct_cnt_at(l) + j] = (uint16_t)r.leaves;
    if (!cnt) return;
    for (int i = 0; i < 8; ++i) {
        if (l == 1) {
            cnt[8] += lab[i] == MLM_OCT_OCC;
            cnt[9] += lab[i] == MLM_OCT_FREE;
        }
        if (r.label == MLM_OCT_INNER) {
            cnt[l - 1] += lab[i] == MLM_OCT_OCC;
            cnt[4 + l - 1] += lab[i] == MLM_OCT_FREE;
        }
    }
}
// Down: cell j of level l (T..1) of the brick whose lower corner has the key kb: an inner cell of the tree writes its row, the rows
// of its leaf children, and hands its children of level l - 1 >= 1 their numbers; any other cell tells them they are not in the tree.
MLM_OCT_HD void mlm_oct_brick_down(MlmOctBrick &B, const MlmOctGeo &G, const MlmOctOut &O, const long long kb[3], int l, int j) {
    int ci[8], x, y, z, lab[8], inner[8], leaves[8], cib[8], clb[8];
    mlm_oct_brick_children(G.T, l, j, ci, x, y, z);
    const int me = mlm_oct_cnt_at(l) + j;
    const bool in_tree = B.lab[mlm_oct_lab_at(l) + j] == MLM_OCT_INNER && B.ib[me] >= 0;
    if (!in_tree) {
        if (l > 1)
            for (int i = 0; i < 8; ++i) B.ib[mlm_oct_cnt_at(l - 1) + ci[i]] = B.lb[mlm_oct_cnt_at(l - 1) + ci[i]] = -1;
        return;
    }
    mlm_oct_brick_gather(B, l, ci, lab, inner, leaves);
    mlm_oct_hand_down(B.ib[me], B.lb[me], inner, leaves, cib, clb);
    unsigned word = 0;
    for (int i = 0; i < 8; ++i) {
        word |= (unsigned)lab[i] << (2 * i);
        if (l > 1) {
            B.ib[mlm_oct_cnt_at(l - 1) + ci[i]] = cib[i];
            B.lb[mlm_oct_cnt_at(l - 1) + ci[i]] = clb[i];
        }
        if (lab[i] == MLM_OCT_OCC || lab[i] == MLM_OCT_FREE)
            mlm_oct_leaf_row(G, O, clb[i], kb[0] + ((long long)(2 * x + mlm_oct_child_x(i)) << (l - 1)),
                             kb[1] + ((long long)(2 * y + mlm_oct_child_y(i)) << (l - 1)), kb[2] + ((long long)(2 * z + mlm_oct_child_z(i)) << (l - 1)),
                             l - 1, lab[i]);
    }
    mlm_oct_inner_row(G, O, B.ib[me], word, kb[0] + ((long long)x << l), kb[1] + ((long long)y << l), kb[2] + ((long long)z << l), l, B.icnt[me]);
}

// ---- the levels above the bricks -------------------------------------------------------------------------------------------------
struct MlmOctUpper {
    uint8_t *lab;
    int32_t *icnt, *lcnt, *ib, *lb;
    unsigned long long *ctrl;
};
// the children of the level-l cell c (l > T): their indices into the upper arrays (-1: the child does not meet the box: NONE) and
// their labels, inner counts and leaf counts
MLM_OCT_HD void mlm_oct_upper_gather(const MlmOctGeo &G, const MlmOctUpper &U, int l, const long long c[3], long long ci[8], int lab[8], int inner[8],
                                     int leaves[8]) {
    for (int i = 0; i < 8; ++i) {
        const long long cc[3] = {2 * c[0] + mlm_oct_child_x(i), 2 * c[1] + mlm_oct_child_y(i), 2 * c[2] + mlm_oct_child_z(i)};
        ci[i] = mlm_oct_cell_index(G, l - 1, cc);
        lab[i] = ci[i] < 0 ? MLM_OCT_NONE : U.lab[ci[i]];
        inner[i] = ci[i] < 0 ? 0 : U.icnt[ci[i]];
        leaves[i] = ci[i] < 0 ? 0 : U.lcnt[ci[i]];
    }
}
// Up: cell j of level l (T < l <= depth) from level l - 1
MLM_OCT_HD void mlm_oct_upper_up(const MlmOctGeo &G, const MlmOctUpper &U, int l, long long j) {
    long long c[3], ci[8];
    int lab[8], inner[8], leaves[8];
    mlm_oct_cell_at(G, l, j, c);
    mlm_oct_upper_gather(G, U, l, c, ci, lab, inner, leaves);
    const MlmOctNode r = mlm_oct_reduce(lab, inner, leaves);
    U.lab[G.off[l] + j] = (uint8_t)r.label;
    U.icnt[G.off[l] + j] = r.inner;
    U.lcnt[G.off[l] + j] = r.leaves;
}
// The root, once every level is reduced: N, M and its label for the summary; it starts the numbering at inner node 0, leaf 0; a root
// that is a leaf is the one leaf of the tree
MLM_OCT_HD void mlm_oct_root(const MlmOctGeo &G, const MlmOctUpper &U) {
    const long long r = G.off[G.depth];
    const int label = U.lab[r];
    U.ctrl[kOctCtrlN] = (unsigned long long)U.icnt[r];
    U.ctrl[kOctCtrlM] = (unsigned long long)U.lcnt[r];
    U.ctrl[kOctCtrlRoot] = (unsigned long long)label;
    U.ib[r] = U.lb[r] = label == MLM_OCT_NONE ? -1 : 0;
    if (label == MLM_OCT_OCC) mlm_oct_count(&U.ctrl[kOctCtrlOccLeaves + G.depth], 1);
    if (label == MLM_OCT_FREE) mlm_oct_count(&U.ctrl[kOctCtrlFreeLeaves + G.depth], 1);
}
// Down: cell j of level l (depth >= l > T) hands its children their numbers (-1 unless it is an inner cell of the tree) and counts its
// leaf children, leaves of level l - 1
MLM_OCT_HD void mlm_oct_upper_down(const MlmOctGeo &G, const MlmOctUpper &U, int l, long long j) {
    long long c[3], ci[8];
    int lab[8], inner[8], leaves[8], cib[8], clb[8];
    mlm_oct_cell_at(G, l, j, c);
    mlm_oct_upper_gather(G, U, l, c, ci, lab, inner, leaves);
    const long long me = G.off[l] + j;
    const bool in_tree = U.lab[me] == MLM_OCT_INNER && U.ib[me] >= 0;
    if (in_tree) mlm_oct_hand_down(U.ib[me], U.lb[me], inner, leaves, cib, clb);
    for (int i = 0; i < 8; ++i) {
        if (ci[i] < 0) continue;
        U.ib[ci[i]] = in_tree ? cib[i] : -1;
        U.lb[ci[i]] = in_tree ? clb[i] : -1;
        if (in_tree && lab[i] == MLM_OCT_OCC) mlm_oct_count(&U.ctrl[kOctCtrlOccLeaves + l - 1], 1);
        if (in_tree && lab[i] == MLM_OCT_FREE) mlm_oct_count(&U.ctrl[kOctCtrlFreeLeaves + l - 1], 1);
    }
}
// the rows of cell j of level l (depth >= l > T) if it is an inner cell of the tree: its own, and those of its leaf children
MLM_OCT_HD void mlm_oct_upper_emit(const MlmOctGeo &G, const MlmOctUpper &U, const MlmOctOut &O, int l, long long j) {
    const long long me = G.off[l] + j;
    if (U.lab[me] != MLM_OCT_INNER || U.ib[me] < 0) return;
    long long c[3], ci[8];
    int lab[8], inner[8], leaves[8];
    mlm_oct_cell_at(G, l, j, c);
    mlm_oct_upper_gather(G, U, l, c, ci, lab, inner, leaves);
    unsigned word = 0;
    for (int i = 0; i < 8; ++i) {
        word |= (unsigned)lab[i] << (2 * i);
        if (lab[i] == MLM_OCT_OCC || lab[i] == MLM_OCT_FREE)
            mlm_oct_leaf_row(G, O, U.lb[ci[i]], (2 * c[0] + mlm_oct_child_x(i)) << (l - 1), (2 * c[1] + mlm_oct_child_y(i)) << (l - 1),
                             (2 * c[2] + mlm_oct_child_z(i)) << (l - 1), l - 1, lab[i]);
    }
    mlm_oct_inner_row(G, O, U.ib[me], word, c[0] << l, c[1] << l, c[2] << l, l, U.icnt[me]);
}
// ... and of a root that is a leaf
MLM_OCT_HD void mlm_oct_root_emit(const MlmOctGeo &G, const MlmOctUpper &U, const MlmOctOut &O) {
    const int label = U.lab[G.off[G.depth]];
    if (label == MLM_OCT_OCC || label == MLM_OCT_FREE) mlm_oct_leaf_row(G, O, 0, 0, 0, 0, G.depth, label);
}
// whether brick b (counted within level T) has rows to write: it is an inner cell of the tree, and an inner node or a leaf of its
// subtree lies in a range that has an array
MLM_OCT_HD bool mlm_oct_brick_wanted(const MlmOctGeo &G, const MlmOctUpper &U, const MlmOctOut &O, long long b) {
    const long long me = G.off[G.T] + b, ib = U.ib[me], lb = U.lb[me];
    if (U.lab[me] != MLM_OCT_INNER || ib < 0) return false;
    const bool inner = (O.words || O.inner4 || O.skip) && ib < O.n1 && ib + U.icnt[me] > O.n0;
    const bool leaves = (O.leaf4 || O.leaf_class) && lb < O.m1 && lb + U.lcnt[me] > O.m0;
    return inner || leaves;
}
// the level of cell j of the upper arrays (off[T] <= j < off[depth + 1])
MLM_OCT_HD int mlm_oct_level_of(const MlmOctGeo &G, long long j) {
    int l = G.T;
    while (l < G.depth && j >= G.off[l + 1]) ++l;
    return l;
}

// ---- plan and argument checks (host) ---------------------------------------------------------------------------------------------
// Scratch of mlm_export_octree, each part starting on a multiple of 256 bytes: per cell of levels T..depth (C cells: per level the
// product over the axes of ((khi - 1) >> l) - (klo >> l) + 1) one label byte and four int32 — inner count, leaf count, first inner
// node, first leaf —, and the control block: up(C) + 4 up(4 C) + 1024.  Nothing is kept per voxel: the levels below a brick's top are
// recomputed where the rows are written.
// why != 0: refused — 1: depth outside 1..31, 2: a dim below 1 or the box not within [-2^(depth-1), 2^(depth-1)) per axis.
struct MlmOctPlan {
    int why, T;
    long long half, bricks, cells;
    long long off[33];
    long long lab_bytes, cnt_bytes, off_icnt, off_lcnt, off_ib, off_lb, off_ctrl, scratch_bytes;
};
inline MlmOctPlan mlm_oct_plan(const long long lo[3], const long long D[3], int depth) {
    MlmOctPlan p{};
    if (depth < 1 || depth > 31) {
        p.why = 1;
        return p;
    }
    p.half = 1ll << (depth - 1);
    for (int a = 0; a < 3; ++a)
        if (D[a] < 1 || lo[a] < -p.half || lo[a] + D[a] > p.half) {
            p.why = 2;
            return p;
        }
    p.T = depth < kOctBrickLevel ? depth : kOctBrickLevel;
    for (int l = p.T; l <= depth; ++l) {
        long long n = 1;
        for (int a = 0; a < 3; ++a) n *= ((lo[a] + D[a] - 1 + p.half) >> l) - ((lo[a] + p.half) >> l) + 1;
        p.off[l] = p.cells;
        p.cells += n;
        if (l == p.T) p.bricks = n;
    }
    p.off[depth + 1] = p.cells;
    auto up = [](long long v) { return (v + 255) & ~255ll; };
    p.lab_bytes = up(p.cells);
    p.cnt_bytes = up(4 * p.cells);
    p.off_icnt = p.lab_bytes;
    p.off_lcnt = p.off_icnt + p.cnt_bytes;
    p.off_ib = p.off_lcnt + p.cnt_bytes;
    p.off_lb = p.off_ib + p.cnt_bytes;
    p.off_ctrl = p.off_lb + p.cnt_bytes;
    p.scratch_bytes = p.off_ctrl + kOctCtrlBytes;
    return p;
}
inline MlmOctGeo mlm_oct_geo(const long long lo[3], const long long D[3], int depth, int flags, const MlmOctPlan &p) {
    MlmOctGeo G{};
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = lo[a];
        G.D[a] = D[a];
        G.klo[a] = lo[a] + p.half;
        G.khi[a] = lo[a] + D[a] + p.half;
    }
    G.half = p.half;
    for (int l = 0; l < 33; ++l) G.off[l] = p.off[l];
    G.depth = depth;
    G.T = p.T;
    G.flags = flags;
    return G;
}
inline MlmOctUpper mlm_oct_upper(void *scratch, const MlmOctPlan &p) {
    char *base = (char *)scratch;
    return MlmOctUpper{(uint8_t *)base, (int32_t *)(base + p.off_icnt), (int32_t *)(base + p.off_lcnt), (int32_t *)(base + p.off_ib),
                       (int32_t *)(base + p.off_lb), (unsigned long long *)(base + p.off_ctrl)};
}

// Argument check of mlm_export_octree beyond the window and the plan: 0 fine, 1 an unknown flag bit, 2 a negative cap, 3 a cap at odds
// with its arrays (a cap is 0 iff all of its arrays are null), 4 no output at all
inline int mlm_oct_args(int flags, long long cap_inner, bool any_inner_array, long long cap_leaves, bool any_leaf_array, bool summary) {
    if (flags & ~(MLM_OCT_F_INFL | MLM_OCT_F_OCC_ONLY)) return 1;
    if (cap_inner < 0 || cap_leaves < 0) return 2;
    if ((cap_inner == 0) == any_inner_array || (cap_leaves == 0) == any_leaf_array) return 3;
    if (!any_inner_array && !any_leaf_array && !summary) return 4;
    return 0;
}

// the summary from the control block as the kernels left it
inline void mlm_oct_summary(const unsigned long long *ctrl, int64_t sm[MLM_OCT_ROW_I64]) {
    for (int i = 0; i < MLM_OCT_ROW_I64; ++i) sm[i] = 0;
    sm[0] = (int64_t)ctrl[kOctCtrlN];
    sm[1] = (int64_t)ctrl[kOctCtrlM];
    for (int l = 0; l < 32; ++l) {
        sm[2] += (int64_t)ctrl[kOctCtrlOccLeaves + l];
        sm[3] += (int64_t)ctrl[kOctCtrlFreeLeaves + l];
        sm[8 + l] = (int64_t)(ctrl[kOctCtrlOccLeaves + l] + ctrl[kOctCtrlFreeLeaves + l]);
    }
    sm[4] = (int64_t)ctrl[kOctCtrlOccVox];
    sm[5] = (int64_t)ctrl[kOctCtrlFreeVox];
    sm[6] = (int64_t)ctrl[kOctCtrlRoot];
}
