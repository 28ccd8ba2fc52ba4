// mlm_kernels_warp.h — the kernels of mlm_warp_blocks (include/mlmap_hip.h; the rule: mlm_warp.h).  Part of mlmap_hip.hip.
//
//  - k_warp_candidates: a lane per source block puts the packed keys of its candidates (mlm_warp_candidates) into an open-addressed
//    set — mlm_mix, linear probing, 64-bit compare-and-swap.  Only membership matters: the atomics cannot change the answer.
//  - k_warp_set_count / k_crop_scan / k_warp_set_list: the used entries of the set compacted into a list by mlm_kernels_crop.h's
//    atomic-free three-phase prefix; the host sorts the list with mlm_sort_pairs_u64_u32 — the candidates in emission order.
//  - k_warp_count: a wave per candidate, lanes over its cells with x fastest, runs the gather for the live predicate and the classes;
//    one ballot and popcount per counter and trip.  A lane keeps the slot of the source block of its previous voxel (MlmWarpSrc): a
//    run of voxels in one source block costs one table probe.  Four counters per candidate; k_warp_sums adds them up for the
//    call — integer adds.
//  - k_warp_emit_count / k_crop_scan / k_warp_emit_list: the candidates with a live voxel numbered by the same prefix.
//  - k_warp_write: a wave per emitted block runs the gather again and stores key and planes into row `rank` — consecutive lanes,
//    consecutive addresses.  The gather's reads are lines through a few source blocks and are left to L2.
// A cell index splits into its coordinates by two multiplications (mlm_host.h: strip_magic; cells < 2^20), by divisions beyond that.
#pragma once
#include "mlm_kernels_crop.h"
#include "mlm_warp.h"

#define MLM_WARP_CTRL_WORDS 4 // ctrl[0] = count of the scan, ctrl[1] = the candidate set overflowed (never: mlm_warp_span)
#define MLM_WARP_SUMS 4       // live voxels, those with occ 'o', occ 'f', infl 'o'

struct MlmWarp {
    MlmWarpPlan W;
    uint32_t cell_m;                 // strip_magic(n), 0: divide
    const unsigned long long *cand;  // [nc] candidate keys, ascending
    unsigned int nc;
    uint32_t *cnt;                   // [nc][4] live, occ 'o', occ 'f', infl 'o'
    const unsigned int *elist;       // [E] the emitted candidates, ascending
};

// the source voxels of the block the gather is in (mlm_warp.h's callable)
struct MlmWarpSrc {
    const MlmDev &P;
    int slot;
    bool whole; // a released block: element 0 answers, infl 'u'
    __device__ __forceinline__ bool operator()(const int g[3], const int c[3], bool new_block, float &lo, uint8_t &occ, uint8_t &infl) {
        if (new_block) {
            slot = mlm_block_find(P, g[0], g[1], g[2]); // (-1 beyond the 21-bit range as well)
            whole = slot >= 0 && P.explore && P.blk_collapsed[slot];
        }
        if (slot < 0) return false;
        const size_t at = (size_t)slot * P.cells + (whole ? (size_t)0 : (size_t)((c[2] * P.n + c[1]) * P.n + c[0]));
        lo = P.log_odds[at];
        occ = P.occ[at];
        infl = whole ? (uint8_t)'u' : P.infl[at];
        return true;
    }
};

struct MlmWarpDiv {
    uint32_t n, m;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return m ? __umulhi(i << 1, m) : i / n; }
};

__device__ __forceinline__ MlmWarpGeom mlm_warp_geom(const MlmDev &P) { return MlmWarpGeom{P.d_sub, P.d_glb, P.d_sub_half, P.n}; }

__global__ __launch_bounds__(MLM_BLOCK) void k_warp_candidates(const MlmDev P, const MlmWarpPlan W, unsigned int nb, unsigned long long *__restrict__ set,
                                                               uint32_t set_mask, unsigned int *__restrict__ ctrl) {
    const MlmWarpGeom G = mlm_warp_geom(P);
    const int *const keys = P.block_keys;
    for (unsigned int s = blockIdx.x * blockDim.x + threadIdx.x; s < nb; s += gridDim.x * blockDim.x) {
        const int g[3] = {keys[3 * (size_t)s], keys[3 * (size_t)s + 1], keys[3 * (size_t)s + 2]};
        int32_t klo[3], khi[3];
        if (!mlm_warp_candidates(W, G, g, klo, khi)) continue;
        for (int x = klo[0]; x <= khi[0]; ++x)
            for (int y = klo[1]; y <= khi[1]; ++y)
                for (int z = klo[2]; z <= khi[2]; ++z) {
                    const int k[3] = {x, y, z};
                    const unsigned long long key = mlm_warp_pack(k);
                    uint32_t at = mlm_mix(key) & set_mask;
                    bool in = false;
                    for (uint32_t probe = 0; probe <= set_mask && !in; ++probe) {
                        const unsigned long long prev = atomicCAS(&set[at], MLM_WARP_EMPTY, key);
                        in = prev == MLM_WARP_EMPTY || prev == key;
                        at = (at + 1) & set_mask;
                    }
                    if (!in) ctrl[1] = 1u;
                }
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_warp_set_count(const unsigned long long *__restrict__ set, unsigned int nt, unsigned int chunks,
                                                              unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_count_chunks([&](unsigned int i) { return set[i] != MLM_WARP_EMPTY; }, nt, chunks, chunk_cnt);
}
__global__ __launch_bounds__(MLM_BLOCK) void k_warp_set_list(const unsigned long long *__restrict__ set, unsigned int nt, unsigned int chunks,
                                                             const unsigned int *__restrict__ chunk_cnt, unsigned long long *__restrict__ list,
                                                             uint32_t *__restrict__ vals, unsigned int cap) {
    mlm_crop_rank_chunks([&](unsigned int i) { return set[i] != MLM_WARP_EMPTY; }, nt, chunks, chunk_cnt, [&](unsigned int i, unsigned int d, bool used) {
        if (used && d < cap) {
            list[d] = set[i];
            vals[d] = d;
        }
    });
}

__global__ __launch_bounds__(MLM_BLOCK) void k_warp_count(const MlmDev P, const MlmWarp Q) {
    const MlmWarpGeom G = mlm_warp_geom(P);
    const MlmWarpDiv div{(uint32_t)P.n, Q.cell_m};
    const uint32_t cells = (uint32_t)P.cells;
    const bool seen = Q.W.seen != 0;
    const unsigned int nc = Q.nc;
    const unsigned long long *const cand = Q.cand;
    uint32_t *const cnt = Q.cnt;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = Q.W.T[i];
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    for (unsigned int i = blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); i < nc; i += waves) {
        int g[3];
        mlm_warp_unpack(cand[i], g);
        uint32_t n_live = 0, n_o = 0, n_f = 0, n_io = 0;
        MlmScoreBlock B{};
        MlmWarpSrc src{P, -1, false};
        for (uint32_t c0 = 0; c0 < cells; c0 += 64) { // (wave-uniform: every lane meets every ballot)
            const uint32_t ci = c0 + (uint32_t)lane;
            int c[3];
            mlm_warp_cell(ci < cells ? ci : 0u, G.n, div, c);
            float lo;
            uint8_t occ, infl;
            const bool live = ci < cells && mlm_warp_voxel(T, seen, G, g, c, src, B, lo, occ, infl);
            n_live += (uint32_t)__builtin_popcountll(__ballot(live));
            n_o += (uint32_t)__builtin_popcountll(__ballot(live && occ == (uint8_t)'o'));
            n_f += (uint32_t)__builtin_popcountll(__ballot(live && occ == (uint8_t)'f'));
            n_io += (uint32_t)__builtin_popcountll(__ballot(live && infl == (uint8_t)'o'));
        }
        if (lane == 0) *(uint4 *)(cnt + 4 * (size_t)i) = make_uint4(n_live, n_o, n_f, n_io);
    }
}

// the call's four sums over the candidates' counters: per lane, per wave (shuffles), per workgroup (LDS), then one add per counter
// and workgroup — integer adds, one value whatever the order (a wave per candidate adding its own counters met on one cache line:
// 0.8 ms of the 1.1 ms the call took on 20 000 candidates)
__global__ __launch_bounds__(MLM_BLOCK) void k_warp_sums(const uint32_t *__restrict__ cnt, unsigned int nc, unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long s_part[MLM_BLOCK / 64][MLM_WARP_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long acc[MLM_WARP_SUMS] = {0, 0, 0, 0};
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc; i += gridDim.x * blockDim.x) {
        const uint4 r = *(const uint4 *)(cnt + 4 * (size_t)i);
        acc[0] += r.x, acc[1] += r.y, acc[2] += r.z, acc[3] += r.w;
    }
#pragma unroll
    for (int k = 0; k < MLM_WARP_SUMS; ++k) {
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off);
        if (lane == 0) s_part[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < MLM_WARP_SUMS) {
        unsigned long long t = 0;
        for (int w = 0; w < MLM_BLOCK / 64; ++w) t += s_part[w][threadIdx.x];
        if (t) atomicAdd(sums + threadIdx.x, t);
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_warp_emit_count(const uint32_t *__restrict__ cnt, unsigned int nc, unsigned int chunks,
                                                               unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_count_chunks([&](unsigned int i) { return cnt[4 * (size_t)i] != 0u; }, nc, chunks, chunk_cnt);
}
__global__ __launch_bounds__(MLM_BLOCK) void k_warp_emit_list(const uint32_t *__restrict__ cnt, unsigned int nc, unsigned int chunks,
                                                              const unsigned int *__restrict__ chunk_cnt, unsigned int *__restrict__ elist) {
    mlm_crop_rank_chunks([&](unsigned int i) { return cnt[4 * (size_t)i] != 0u; }, nc, chunks, chunk_cnt, [&](unsigned int i, unsigned int d, bool emitted) {
        if (emitted && d < nc) elist[d] = i; // (always: d counts emitted candidates below i)
    });
}

// output rows [r0, r1): row r holds emitted block r; the arrays start at row r0 (any of them may be null)
__global__ __launch_bounds__(MLM_BLOCK) void k_warp_write(const MlmDev P, const MlmWarp Q, unsigned int r0, unsigned int r1, int32_t *__restrict__ keys,
                                                          float *__restrict__ lo_out, uint8_t *__restrict__ occ_out, uint8_t *__restrict__ infl_out) {
    const MlmWarpGeom G = mlm_warp_geom(P);
    const MlmWarpDiv div{(uint32_t)P.n, Q.cell_m};
    const uint32_t cells = (uint32_t)P.cells;
    const bool seen = Q.W.seen != 0;
    const unsigned int nc = Q.nc;
    const unsigned long long *const cand = Q.cand;
    const unsigned int *const elist = Q.elist;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = Q.W.T[i];
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const bool planes = lo_out || occ_out || infl_out;
    for (unsigned int r = r0 + blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); r < r1; r += waves) {
        const unsigned int i = elist[r];
        if (i >= nc) continue; // (never: see k_warp_emit_list)
        int g[3];
        mlm_warp_unpack(cand[i], g);
        const size_t o = (size_t)(r - r0);
        if (keys && lane < 3) keys[3 * o + lane] = lane == 0 ? g[0] : (lane == 1 ? g[1] : g[2]);
        if (!planes) continue;
        MlmScoreBlock B{};
        MlmWarpSrc src{P, -1, false};
        for (uint32_t ci = (uint32_t)lane; ci < cells; ci += 64) {
            int c[3];
            mlm_warp_cell(ci, G.n, div, c);
            float lo;
            uint8_t occ, infl;
            mlm_warp_voxel(T, seen, G, g, c, src, B, lo, occ, infl);
            if (lo_out) lo_out[o * cells + ci] = lo;
            if (occ_out) occ_out[o * cells + ci] = occ;
            if (infl_out) infl_out[o * cells + ci] = infl;
        }
    }
}
