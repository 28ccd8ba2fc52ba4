// mlm_kernels_octree.h — exact pruned occupancy octree of a voxel box (mlm_export_octree; no reference counterpart: the reference
// publishes point markers; labels, tree and numbering are defined in include/mlmap_hip.h on the classes mlm_export_window reads
// out).  The rules are those of mlm_octree.h, which the CPU test driver runs too; here they meet the map and the lanes.
//  - k_oct_up:         a workgroup per brick (a level-T cell of the key lattice, 16^3 voxels, that meets the box): the classes of its
//                      voxels into LDS — the brick spans parts of several map blocks; their slots are looked up once, by as many lanes,
//                      into an LDS table, and the voxel -> (block, cell) split of the brick's 16 coordinates per axis is made once —,
//                      levels 1..T reduced in LDS, the top's label, inner count and leaf count stored, the summary's counters summed
//                      in registers, then LDS, then one atomic per counter and workgroup;
//  - k_oct_tail:       one workgroup: levels T+1..depth reduced level by level (a level has an eighth of the cells below it), the
//                      root's numbers set, then levels depth..T+1 hand the numbers down to the bricks;
//  - k_oct_emit_upper: a lane per cell above the bricks: an inner cell of the tree writes its row and those of its leaf children;
//  - k_oct_emit:       a workgroup per brick that is an inner cell of the tree and holds a row of the range asked for: the pyramid is
//                      rebuilt in LDS as k_oct_up built it (nothing below a brick's top is stored: recomputed), levels T..1 hand the
//                      numbers down in LDS and write the rows.
// No atomic takes part in a number: the numbering is an exclusive prefix over eight children, top-down.
#pragma once
#include "mlm_octree.h"
#include "mlm_kernels_window.h"

constexpr int kOctSlots = 4096;                // map blocks a brick can meet: at most 15 / subbox_n + 2 <= 16 per axis
constexpr int kOctCollapsed = 1 << 30;         // a tabled slot's flag "released block: element 0 answers"
constexpr unsigned int kOctGrid = 1u << 16;    // most workgroups of k_oct_up / k_oct_emit (grid-stride over the bricks)

struct MlmOctLoad {
    int slot[kOctSlots];        // slot of the map block (| kOctCollapsed), -1 absent
    int tg[3][16], tc[3][16];   // per axis and brick coordinate: map block (counted from g0; -1 outside the box), cell coordinate
    long long g0[3];
    int nbk[3];
};

__device__ __forceinline__ long long mlm_oct_floor_div(long long v, int n) { return v >= 0 ? v / n : -((-v + n - 1) / n); }

// the labels of the voxels of the brick at level-T cell cb into B.lab (level 0); ends with a barrier
__device__ __forceinline__ void mlm_oct_brick_load(const MlmDev &P, const MlmOctGeo &G, const long long cb[3], MlmOctBrick &B, MlmOctLoad &S) {
    const int n = P.n, T = G.T, side = 1 << T, flags = G.flags;
    if (threadIdx.x < 48) {
        const int a = threadIdx.x >> 4, i = threadIdx.x & 15;
        const long long v0 = (cb[a] << T) - G.half, v = v0 + i;
        const long long first = max(v0, G.lo[a]), last = min(v0 + side, G.lo[a] + G.D[a]) - 1; // (the brick meets the box: first <= last)
        const long long g0 = mlm_oct_floor_div(first, n);
        const bool inside = i < side && v >= first && v <= last;
        const long long g = inside ? mlm_oct_floor_div(v, n) : 0;
        S.tg[a][i] = (int)(inside ? g - g0 : -1);
        S.tc[a][i] = (int)(inside ? v - g * n : 0);
        if (i == 0) {
            S.g0[a] = g0;
            S.nbk[a] = (int)(mlm_oct_floor_div(last, n) - g0 + 1);
        }
    }
    __syncthreads();
    const int nb0 = S.nbk[0], nb1 = S.nbk[1], nb = nb0 * nb1 * S.nbk[2];
    for (int t = threadIdx.x; t < nb; t += blockDim.x) {
        const int row = t / nb0, ix = t - row * nb0, iz = row / nb1, iy = row - iz * nb1;
        const int slot = mlm_block_find(P, mlm_win_key(S.g0[0] + ix), mlm_win_key(S.g0[1] + iy), mlm_win_key(S.g0[2] + iz));
        S.slot[t] = slot >= 0 && P.explore && P.blk_collapsed[slot] ? slot | kOctCollapsed : slot;
    }
    __syncthreads();
    const int nvox = 1 << (3 * T);
    for (int j = threadIdx.x; j < nvox; j += blockDim.x) {
        const int x = j & (side - 1), y = (j >> T) & (side - 1), z = j >> (2 * T);
        const int gx = S.tg[0][x], gy = S.tg[1][y], gz = S.tg[2][z];
        int label = MLM_OCT_NONE;
        if (gx >= 0 && gy >= 0 && gz >= 0) {
            const int tabled = S.slot[(gz * nb1 + gy) * nb0 + gx];
            const bool collapsed = tabled >= 0 && (tabled & kOctCollapsed);
            const int slot = tabled >= 0 ? tabled & ~kOctCollapsed : -1;
            const size_t at = (size_t)(slot >= 0 ? slot : 0) * P.cells + (collapsed ? 0 : (S.tc[2][z] * n + S.tc[1][y]) * n + S.tc[0][x]);
            label = mlm_oct_class(mlm_win_occ(P, slot, at), mlm_win_infl(P, slot, collapsed, at), flags);
        }
        B.lab[j] = (uint8_t)label;
    }
    __syncthreads();
}

// levels 1..T of the brick from its voxels' labels; ends with a barrier
__device__ __forceinline__ void mlm_oct_brick_reduce(MlmOctBrick &B, int T, unsigned *cnt) {
    for (int l = 1; l <= T; ++l) {
        const int cells = 1 << (3 * (T - l));
        for (int j = threadIdx.x; j < cells; j += blockDim.x) mlm_oct_brick_up(B, T, l, j, cnt);
        __syncthreads();
    }
}

// brick b (counted within level T) -> its level-T cell
__device__ __forceinline__ void mlm_oct_brick_at(const MlmOctGeo &G, long long b, long long cb[3]) { mlm_oct_cell_at(G, G.T, b, cb); }

__global__ __launch_bounds__(MLM_BLOCK) void k_oct_up(const MlmDev P, const MlmOctGeo G, const MlmOctUpper U) {
    __shared__ MlmOctBrick B;
    __shared__ MlmOctLoad S;
    __shared__ unsigned s_cnt[10];
    const int T = G.T;
    const long long bricks = G.off[T + 1] - G.off[T];
    if (threadIdx.x < 10) s_cnt[threadIdx.x] = 0;
    unsigned cnt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long b = blockIdx.x; b < bricks; b += gridDim.x) {
        long long cb[3];
        mlm_oct_brick_at(G, b, cb);
        mlm_oct_brick_load(P, G, cb, B, S); // (its first barrier: the previous brick's top has been read)
        mlm_oct_brick_reduce(B, T, cnt);
        if (threadIdx.x == 0) {
            U.lab[G.off[T] + b] = B.lab[mlm_oct_lab_at(T)];
            U.icnt[G.off[T] + b] = B.icnt[mlm_oct_cnt_at(T)];
            U.lcnt[G.off[T] + b] = B.lcnt[mlm_oct_cnt_at(T)];
        }
    }
    __syncthreads();
    for (int i = 0; i < 10; ++i)
        if (cnt[i]) atomicAdd(&s_cnt[i], cnt[i]);
    __syncthreads();
    if (threadIdx.x < 10 && s_cnt[threadIdx.x]) {
        const int i = threadIdx.x;
        const int at = i < 4 ? kOctCtrlOccLeaves + i : i < 8 ? kOctCtrlFreeLeaves + i - 4 : i == 8 ? kOctCtrlOccVox : kOctCtrlFreeVox;
        atomicAdd(&U.ctrl[at], (unsigned long long)s_cnt[i]);
    }
}

// one workgroup; a barrier orders a level's stores before the next level's loads
__global__ __launch_bounds__(MLM_BLOCK) void k_oct_tail(const MlmOctGeo G, const MlmOctUpper U) {
    const int T = G.T, depth = G.depth;
    for (int l = T + 1; l <= depth; ++l) {
        const long long cells = G.off[l + 1] - G.off[l];
        for (long long j = threadIdx.x; j < cells; j += blockDim.x) mlm_oct_upper_up(G, U, l, j);
        __threadfence();
        __syncthreads();
    }
    if (threadIdx.x == 0) mlm_oct_root(G, U);
    __threadfence();
    __syncthreads();
    for (int l = depth; l > T; --l) {
        const long long cells = G.off[l + 1] - G.off[l];
        for (long long j = threadIdx.x; j < cells; j += blockDim.x) mlm_oct_upper_down(G, U, l, j);
        __threadfence();
        __syncthreads();
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_oct_emit_upper(const MlmOctGeo G, const MlmOctUpper U, const MlmOctOut O) {
    if (blockIdx.x == 0 && threadIdx.x == 0) mlm_oct_root_emit(G, U, O);
    const long long first = G.off[G.T + 1], cells = G.off[G.depth + 1];
    for (long long j = first + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < cells; j += (long long)gridDim.x * blockDim.x) {
        const int l = mlm_oct_level_of(G, j);
        mlm_oct_upper_emit(G, U, O, l, j - G.off[l]);
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_oct_emit(const MlmDev P, const MlmOctGeo G, const MlmOctUpper U, const MlmOctOut O) {
    __shared__ MlmOctBrick B;
    __shared__ MlmOctLoad S;
    const int T = G.T;
    const long long bricks = G.off[T + 1] - G.off[T];
    for (long long b = blockIdx.x; b < bricks; b += gridDim.x) {
        if (!mlm_oct_brick_wanted(G, U, O, b)) continue; // (uniform: every lane reads the same words)
        const long long me = G.off[T] + b;
        const int32_t ib = U.ib[me], lb = U.lb[me];
        long long cb[3];
        mlm_oct_brick_at(G, b, cb);
        mlm_oct_brick_load(P, G, cb, B, S); // (its first barrier: the previous brick's rows are written)
        mlm_oct_brick_reduce(B, T, nullptr);
        if (threadIdx.x == 0) {
            B.ib[mlm_oct_cnt_at(T)] = ib;
            B.lb[mlm_oct_cnt_at(T)] = lb;
        }
        __syncthreads();
        const long long kb[3] = {cb[0] << T, cb[1] << T, cb[2] << T};
        for (int l = T; l >= 1; --l) {
            const int cells = 1 << (3 * (T - l));
            for (int j = threadIdx.x; j < cells; j += blockDim.x) mlm_oct_brick_down(B, G, O, kb, l, j);
            __syncthreads();
        }
    }
}
