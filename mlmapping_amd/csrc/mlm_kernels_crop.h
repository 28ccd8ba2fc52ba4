// mlm_kernels_crop.h — the kernels of mlm_crop_blocks (include/mlmap_hip.h; the rule: mlm_crop.h).  Part of mlmap_hip.hip.
//
//  - k_crop_count / k_crop_scan / k_crop_list: the drop flag of every slot in use from its block key, an exclusive prefix over the
//    slots in three phases (flags counted per chunk of MLM_CROP_SLOTS_PER_CHUNK slots; the chunk counts scanned by one workgroup; every
//    slot ranked inside its chunk by ballots) with no atomic in it, and the list of mlm_crop.h: dropped slots in front, kept slots behind.
//    The host reads D and H (ctrl[0], ctrl[1]) once.
//  - k_crop_page: a wave per dropped block copies its key, its three planes and its released flag to output row d(s).  It runs before
//    the move: the holes are among its sources.
//  - k_crop_move: a wave per (hole, filler) pair copies what grow_pool carries over of a block — key, log-odds, occupancy, inflated
//    occupancy, and in frontier mode the frontier flags and the block's released / observed flags — from the filler's slot to the hole's.
//    Everything else of a slot is per-frame scratch that is at its initial value while nothing is in flight.
// The two copy kernels move 16 bytes per lane where a block's rows are 16-byte aligned, else a dword or a byte: the widths are
// template parameters the host chooses per handle (mlm_crop_float_width / mlm_crop_byte_width) and, for k_crop_page, per destination.
#pragma once
#include "mlm_crop.h"

#define MLM_CROP_CTRL_WORDS 4 // ctrl[0] = D, ctrl[1] = H

__device__ __forceinline__ bool mlm_crop_slot_drops(const MlmDev &P, const MlmCropBox &B, unsigned int s) {
    return mlm_crop_drops(B, P.block_keys[3 * (size_t)s], P.block_keys[3 * (size_t)s + 1], P.block_keys[3 * (size_t)s + 2]);
}

// The first and the third phase of the prefix over any flag of the items [0, nb) (mlm_warp_blocks numbers its candidates with them too).
// phase 1: flagged items of every chunk; pred(s) for s < nb
template <class Pred>
__device__ __forceinline__ void mlm_crop_count_chunks(Pred pred, unsigned int nb, unsigned int chunks, unsigned int *__restrict__ chunk_cnt) {
    __shared__ unsigned int s_wave[MLM_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long s0 = (unsigned long long)c * MLM_CROP_SLOTS_PER_CHUNK;
        unsigned int mine = 0;
        // (whole workgroups stay in the loop: ballots and barriers see every lane)
        for (unsigned int r = 0; r < MLM_CROP_SLOTS_PER_CHUNK; r += MLM_BLOCK) {
            const unsigned long long s = s0 + r + threadIdx.x;
            const bool drop = s < nb && pred((unsigned int)s);
            mine += (unsigned int)__builtin_popcountll(__ballot(drop));
        }
        __syncthreads(); // (the previous chunk's wave counts are read)
        if (lane == 0) s_wave[wave] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int t = 0;
            for (int w = 0; w < MLM_BLOCK / 64; ++w) t += s_wave[w];
            chunk_cnt[c] = t;
        }
    }
}
// phase 3 (chunk_cnt scanned by k_crop_scan): emit(s, d, flag) for every s < nb, d the number of flagged items below s
template <class Pred, class Emit>
__device__ __forceinline__ void mlm_crop_rank_chunks(Pred pred, unsigned int nb, unsigned int chunks, const unsigned int *__restrict__ chunk_cnt, Emit emit) {
    __shared__ unsigned int s_wave[MLM_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long s0 = (unsigned long long)c * MLM_CROP_SLOTS_PER_CHUNK;
        unsigned int base = chunk_cnt[c];
        for (unsigned int r = 0; r < MLM_CROP_SLOTS_PER_CHUNK; r += MLM_BLOCK) {
            const unsigned long long s = s0 + r + threadIdx.x;
            const bool live = s < nb;
            const bool drop = live && pred((unsigned int)s);
            const unsigned long long bal = __ballot(drop);
            __syncthreads(); // (the previous round's wave totals are read)
            if (lane == 0) s_wave[wave] = (unsigned int)__builtin_popcountll(bal);
            __syncthreads();
            unsigned int before = 0, total = 0;
            for (int w = 0; w < MLM_BLOCK / 64; ++w) {
                if (w < wave) before += s_wave[w];
                total += s_wave[w];
            }
            if (live) emit((unsigned int)s, base + before + (unsigned int)__builtin_popcountll(bal & ((1ull << lane) - 1ull)), drop);
            base += total;
        }
    }
}

// phase 1: dropped slots of every chunk
__global__ __launch_bounds__(MLM_BLOCK) void k_crop_count(const MlmDev P, const MlmCropBox B, unsigned int nb, unsigned int chunks,
                                                          unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_count_chunks([&](unsigned int s) { return mlm_crop_slot_drops(P, B, s); }, nb, chunks, chunk_cnt);
}

// phase 2: exclusive scan of the chunk counts in place, by one workgroup; the total is D
__global__ __launch_bounds__(MLM_BLOCK) void k_crop_scan(unsigned int *__restrict__ chunk_cnt, unsigned int chunks, unsigned int *__restrict__ ctrl) {
    __shared__ unsigned int s_scan[MLM_BLOCK];
    unsigned int carry = 0;
    for (unsigned int b = 0; b < chunks; b += MLM_BLOCK) {
        const unsigned int c = b + threadIdx.x;
        const unsigned int v = c < chunks ? chunk_cnt[c] : 0u;
        __syncthreads(); // (the previous round's sums are read)
        s_scan[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < MLM_BLOCK; d <<= 1) {
            const unsigned int add = threadIdx.x >= (unsigned int)d ? s_scan[threadIdx.x - d] : 0u;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < chunks) chunk_cnt[c] = carry + s_scan[threadIdx.x] - v; // (D <= nb < 2^31)
        carry += s_scan[MLM_BLOCK - 1];
    }
    if (threadIdx.x == 0) ctrl[0] = carry;
}

// phase 3: d(s) of every slot -> its place in the list; the slot K = nb - D reports H = d(K)
__global__ __launch_bounds__(MLM_BLOCK) void k_crop_list(const MlmDev P, const MlmCropBox B, unsigned int nb, unsigned int chunks,
                                                         const unsigned int *__restrict__ chunk_cnt, unsigned int *__restrict__ ctrl,
                                                         unsigned int *__restrict__ list) {
    const unsigned int D = ctrl[0], K = nb - min(D, nb);
    mlm_crop_rank_chunks([&](unsigned int s) { return mlm_crop_slot_drops(P, B, s); }, nb, chunks, chunk_cnt, [&](unsigned int s, unsigned int d, bool drop) {
        const unsigned int at = mlm_crop_list_pos(s, d, drop, D);
        if (at < nb) list[at] = s; // (always: the list is a permutation of the slots; the bound is the array's)
        if (s == K) ctrl[1] = d;
    });
}

// `bytes` from src to dst by one wave, W bytes per lane and trip (both W-byte aligned, bytes a multiple of W)
template <int W> __device__ __forceinline__ void mlm_crop_copy(void *__restrict__ dst, const void *__restrict__ src, size_t bytes, int lane) {
    using T = typename std::conditional<W == 16, uint4, typename std::conditional<W == 4, uint32_t, uint8_t>::type>::type;
    const size_t n = bytes / W;
    T *__restrict__ d = (T *)dst;
    const T *__restrict__ s = (const T *)src;
    for (size_t i = (size_t)lane; i < n; i += 64) d[i] = s[i];
}

// output rows [r0, r1): row r holds the block of slot list[r]; the arrays start at row r0 (any of them may be null)
template <int FW, int BW>
__global__ __launch_bounds__(MLM_BLOCK) void k_crop_page(const MlmDev P, const unsigned int *__restrict__ list, unsigned int nb, unsigned int r0,
                                                         unsigned int r1, int32_t *__restrict__ keys, float *__restrict__ lo,
                                                         uint8_t *__restrict__ occ, uint8_t *__restrict__ infl, uint8_t *__restrict__ col) {
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    for (unsigned int r = r0 + blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); r < r1; r += waves) {
        const unsigned int s = list[r];
        if (s >= nb) continue; // (never: see k_crop_list)
        const size_t o = (size_t)(r - r0);
        if (keys && lane < 3) keys[3 * o + lane] = P.block_keys[3 * (size_t)s + lane];
        if (col && lane == 3) col[o] = P.explore ? P.blk_collapsed[s] : (uint8_t)0;
        if (lo) mlm_crop_copy<FW>(lo + o * C, P.log_odds + (size_t)s * C, C * sizeof(float), lane);
        if (occ) mlm_crop_copy<BW>(occ + o * C, P.occ + (size_t)s * C, C, lane);
        if (infl) mlm_crop_copy<BW>(infl + o * C, P.infl + (size_t)s * C, C, lane);
    }
}

// pair j < H: the block of slot list[D + (K - H) + j] (>= K) moves to slot list[j] (< K)
template <int FW, int BW>
__global__ __launch_bounds__(MLM_BLOCK) void k_crop_move(const MlmDev P, const unsigned int *__restrict__ list, unsigned int nb, unsigned int D,
                                                         unsigned int K, unsigned int H) {
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    for (unsigned int j = blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); j < H; j += waves) {
        const unsigned int dst = list[mlm_crop_hole_at(j)], src = list[mlm_crop_filler_at(j, D, K, H)];
        if (dst >= K || src < K || src >= nb) continue; // (never: the rule's sources and destinations; nothing is written outside [0, K))
        if (lane < 3) P.block_keys[3 * (size_t)dst + lane] = P.block_keys[3 * (size_t)src + lane];
        mlm_crop_copy<FW>(P.log_odds + (size_t)dst * C, P.log_odds + (size_t)src * C, C * sizeof(float), lane);
        mlm_crop_copy<BW>(P.occ + (size_t)dst * C, P.occ + (size_t)src * C, C, lane);
        mlm_crop_copy<BW>(P.infl + (size_t)dst * C, P.infl + (size_t)src * C, C, lane);
        if (P.explore) {
            mlm_crop_copy<BW>(P.frnt + (size_t)dst * C, P.frnt + (size_t)src * C, C, lane);
            if (lane == 3) P.blk_collapsed[dst] = P.blk_collapsed[src];
            if (lane == 4) P.blk_observed[dst] = P.blk_observed[src];
        }
    }
}
