// mlm_kernels_age.h — the kernels of mlm_age_blocks (include/mlmap_hip.h; the rule: mlm_age.h).  Part of mlmap_hip.hip.
//
//  - k_age_apply<V, DRY>: a wave takes whole blocks (pool slots), several per wave under the grid cap.  The selection predicate is
//    scalar, from the block's key: a block that is not selected costs that key read, its state word and — where asked for — its
//    per_block row, and nothing of its planes.  For a selected block a lane takes V voxels per trip (V = 4: one 16-byte load of
//    log-odds and a dword each of occ and infl — the pool's rows are aligned where cells % 4 == 0; V = 1: the narrow path of cells not
//    divisible by 4 and of blocks with fewer cells than a wave has lanes), runs mlm_age.h's rule and stores only a vector or dword whose
//    bits changed; DRY removes every store into the map.  The eight voxel counts are summed per lane, reduced per wave for per_block,
//    kept in the lane across blocks, reduced per workgroup at the end and written as one row of twelve partial sums, which
//    k_fuse_sums adds up — integer adds, one value whatever the order, and no atomic.  Per block the wave writes its state
//    (MLM_AGE_B_*) into the scratch: the flag the drop is ranked by.
//  - k_age_count / k_crop_scan / k_age_list: mlm_kernels_crop.h's atomic-free three-phase prefix over "state == MLM_AGE_B_EMPTY", and
//    the list of mlm_crop.h — the slots to drop in front, the kept ones behind — that k_crop_move takes.
#pragma once
#include "mlm_age.h"
#include "mlm_kernels_crop.h"
#include "mlm_kernels_fuse.h"

static_assert(MLM_AGE_SUMS == MLM_FUSE_SUMS, "k_fuse_sums adds the partial rows of k_age_apply up");

struct MlmAge {
    MlmAgeRule A;
    MlmAgeSel S;
    unsigned int nb;          // blocks in use
    uint32_t *state;          // [nb] MLM_AGE_B_*
    int32_t *per_block;       // [nb][4] or null
    unsigned long long *part; // [workgroups of k_age_apply][12] partial sums: [0] empty selected blocks, [1] selected blocks, [4 ..] the voxel counts
};

template <int V, bool DRY> __global__ __launch_bounds__(MLM_BLOCK) void k_age_apply(const MlmDev P, const MlmAge G) {
    using FT = typename std::conditional<V == 4, float4, float>::type;
    using BT = typename std::conditional<V == 4, uint32_t, uint8_t>::type;
    const int lane = threadIdx.x & 63;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (scalar: the key reads and the predicate are too)
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    const MlmAgeRule A = G.A;
    unsigned long long acc[MLM_AGE_SUMS] = {};
    for (unsigned int s = blockIdx.x * (MLM_BLOCK / 64) + wave; s < G.nb; s += waves) {
        const int32_t *key = P.block_keys + 3 * (size_t)s;
        const bool selected = mlm_age_selects(G.S, key[0], key[1], key[2]);
        uint32_t cnt[8] = {};
        bool full = false; // a voxel of this lane leaves the block non-empty
        if (selected) {
            FT *la = (FT *)(P.log_odds + (size_t)s * C);
            BT *oa = (BT *)(P.occ + (size_t)s * C), *ia = (BT *)(P.infl + (size_t)s * C);
            for (size_t i = (size_t)lane; i < C / V; i += 64) {
                const FT va = la[i];
                const BT wa = oa[i], xa = ia[i];
                float L[V];
                uint8_t o[V], f[V];
#pragma unroll
                for (int k = 0; k < V; ++k)
                    L[k] = ((const float *)&va)[k], o[k] = (uint8_t)((uint32_t)wa >> (8 * k)), f[k] = (uint8_t)((uint32_t)xa >> (8 * k));
                uint32_t any = 0;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const uint32_t ev = mlm_age_voxel(A, L[k], o[k], f[k]);
                    any |= ev;
                    full = full || !mlm_age_voxel_empty(L[k], o[k], f[k]);
#pragma unroll
                    for (int b = 0; b < 8; ++b) cnt[b] += (ev >> b) & 1u;
                }
                if (!DRY) {
                    if (any & MLM_AGE_E_LO) {
                        FT out;
#pragma unroll
                        for (int k = 0; k < V; ++k) ((float *)&out)[k] = L[k];
                        la[i] = out;
                    }
                    if (any & MLM_AGE_E_OCC) {
                        uint32_t w = 0;
#pragma unroll
                        for (int k = 0; k < V; ++k) w |= (uint32_t)o[k] << (8 * k);
                        oa[i] = (BT)w;
                    }
                    if (any & MLM_AGE_E_INFL_ST) {
                        uint32_t w = 0;
#pragma unroll
                        for (int k = 0; k < V; ++k) w |= (uint32_t)f[k] << (8 * k);
                        ia[i] = (BT)w;
                    }
                }
            }
        }
        // (wave-uniform from here: every lane meets the ballot and every shuffle)
        const bool empty = selected && __ballot(full) == 0ull;
        const int32_t state = !selected ? MLM_AGE_B_UNSELECTED : empty ? MLM_AGE_B_EMPTY : MLM_AGE_B_KEPT;
        if (G.per_block) {
            uint32_t aged = 0, forgot = 0, turned = 0;
            if (selected) aged = mlm_fuse_wave_sum(cnt[0]), forgot = mlm_fuse_wave_sum(cnt[2]), turned = mlm_fuse_wave_sum(cnt[5] + cnt[6]);
            if (lane == 0) { // (a caller's array need not be 16-byte aligned)
                int32_t *const pb = G.per_block + MLM_AGE_PB * (size_t)s;
                pb[0] = (int32_t)aged, pb[1] = (int32_t)forgot, pb[2] = (int32_t)turned, pb[3] = state;
            }
        }
        if (lane == 0) {
            G.state[s] = (uint32_t)state;
            acc[0] += empty;
            acc[1] += selected;
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[4 + b] += cnt[b];
    }
    // per wave (shuffles), per workgroup (LDS), then one row of partial sums per workgroup — plain stores; k_fuse_sums adds the rows up
    __shared__ unsigned long long s_part[MLM_BLOCK / 64][MLM_AGE_SUMS];
#pragma unroll
    for (int k = 0; k < MLM_AGE_SUMS; ++k) {
        unsigned long long v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) s_part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < MLM_AGE_SUMS) {
        unsigned long long t = 0;
        for (int w = 0; w < MLM_BLOCK / 64; ++w) t += s_part[w][threadIdx.x];
        G.part[(size_t)blockIdx.x * MLM_AGE_SUMS + threadIdx.x] = t;
    }
}

// the drop set of MLM_AGE_DROP — the empty selected blocks — counted per chunk, and ranked into the list of mlm_crop.h
__global__ __launch_bounds__(MLM_BLOCK) void k_age_count(const uint32_t *__restrict__ state, unsigned int nb, unsigned int chunks,
                                                         unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_count_chunks([&](unsigned int s) { return state[s] == (uint32_t)MLM_AGE_B_EMPTY; }, nb, chunks, chunk_cnt);
}
__global__ __launch_bounds__(MLM_BLOCK) void k_age_list(const uint32_t *__restrict__ state, unsigned int nb, unsigned int chunks,
                                                        const unsigned int *__restrict__ chunk_cnt, unsigned int *__restrict__ ctrl,
                                                        unsigned int *__restrict__ list) {
    const unsigned int D = ctrl[0], K = nb - min(D, nb);
    mlm_crop_rank_chunks([&](unsigned int s) { return state[s] == (uint32_t)MLM_AGE_B_EMPTY; }, nb, chunks, chunk_cnt, [&](unsigned int s, unsigned int d, bool drop) {
        const unsigned int at = mlm_crop_list_pos(s, d, drop, D);
        if (at < nb) list[at] = s; // (always: the list is a permutation of the slots; the bound is the array's)
        if (s == K) ctrl[1] = d;
    });
}
