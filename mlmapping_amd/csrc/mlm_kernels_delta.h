// mlm_kernels_delta.h — the kernels of mlm_delta_blocks (include/mlmap_hip.h; the rule: mlm_delta.h).  Part of mlmap_hip.hip.
//
//  - k_delta_digest<V>: a wave takes whole blocks (pool slots), several per wave under the grid cap.  The wave index goes through
//    readfirstlane: the key loads and the box predicate are scalar, and a block that is not selected costs its key read and the "no
//    key" entry of the sort.  For a selected block a lane takes V voxels per trip (V = 4: one 16-byte load of log-odds and a dword each
//    of occ and infl; V = 1: the narrow path of cells not divisible by 4 and of blocks with fewer cells than a wave has lanes), adds
//    mlm_delta.h's two terms per voxel — four 64-bit multiplies; (c + 1) * GOLD advances by an add — into two uint64 per lane, which
//    shuffles reduce.  No LDS and no atomic in the digest.  Per slot the wave writes the packed key and the slot for the sort, the two
//    digest words and the empty ballot (mlm_age.h's predicate); per workgroup one row of partial counts, which k_fuse_sums adds up.
//  - the host sorts (packed key, slot) with mlm_sort_pairs_u64_u32: the selected blocks in table order in front, the others behind.
//  - k_delta_join: a lane per sorted live block finds its key in the previous table by binary search and classifies the block; a lane
//    per previous row checks its range and its order against its neighbour, and — inside the box — finds its key among the live keys.
//    Per workgroup one more row of partial counts.
//  - k_delta_count / k_crop_scan / k_delta_rank: mlm_kernels_crop.h's atomic-free three-phase prefix over "changed or new" and over
//    "gone": the lists of the emitted blocks and of the gone rows, ascending.
//  - k_delta_rows: the table rows, the gone keys.  k_delta_emit<FW, BW>: a wave per emitted block writes key, kind and the planes of the
//    view — 16 bytes per lane where source and destination rows are aligned, else a dword or a byte; a released block is expanded from
//    its element 0.
#pragma once
#include "mlm_delta.h"
#include "mlm_kernels_crop.h"
#include "mlm_kernels_fuse.h"

static_assert(MLM_DELTA_SUMS == MLM_FUSE_SUMS, "k_fuse_sums adds the partial rows of k_delta_digest and k_delta_join up");

#define MLM_DELTA_CTRL_WORDS 4 // ctrl[0] = emitted blocks, ctrl[1] = gone rows (k_crop_scan), ctrl[2] = a previous key out of range, ctrl[3] = out of order
// columns of a partial row (and of the sums): the digest's
#define MLM_DELTA_S_EMPTY 0
#define MLM_DELTA_S_SELECTED 1
// ... and the join's
#define MLM_DELTA_S_INBOX 2
#define MLM_DELTA_S_KIND 3 // + MLM_DELTA_K_*: unchanged, changed, new
#define MLM_DELTA_S_GONE 6

struct MlmDelta {
    MlmAgeSel S;
    unsigned int nb, n_prev;           // blocks in use; rows of the previous table
    int32_t no_infl;                   // MLM_DELTA_NO_INFL
    const int32_t *prev_keys;          // [n_prev][3]
    const unsigned long long *prev_dg; // [n_prev][2]
    unsigned long long *packed;        // [nb] by slot: the packed key, MLM_WARP_EMPTY where not selected
    uint32_t *slot_of;                 // [nb] by slot: the slot (the sort's value)
    const unsigned long long *sorted;  // [nb] the packed keys, ascending
    const uint32_t *sorted_slot;       // [nb] their slots
    unsigned long long *dg;            // [nb][2] by slot
    uint32_t *kind;                    // [nb] by sorted position: MLM_DELTA_K_*
    uint32_t *pstate;                  // [n_prev] MLM_DELTA_P_*
    unsigned int *elist, *glist;       // the emitted sorted positions; the gone rows
    unsigned long long *part;          // [workgroups of k_delta_digest + of k_delta_join][12] partial counts
};

// one row of partial counts per workgroup from what every lane counted: per wave (shuffles), per workgroup (LDS), plain stores
__device__ __forceinline__ void mlm_delta_part_row(const unsigned long long (&acc)[MLM_DELTA_SUMS], unsigned long long *__restrict__ row) {
    __shared__ unsigned long long s_part[MLM_BLOCK / 64][MLM_DELTA_SUMS];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < MLM_DELTA_SUMS; ++k) {
        unsigned long long v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) s_part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < MLM_DELTA_SUMS) {
        unsigned long long t = 0;
        for (int w = 0; w < MLM_BLOCK / 64; ++w) t += s_part[w][threadIdx.x];
        row[threadIdx.x] = t;
    }
}

template <int V> __global__ __launch_bounds__(MLM_BLOCK) void k_delta_digest(const MlmDev P, const MlmDelta D) {
    using FT = typename std::conditional<V == 4, float4, float>::type;
    using BT = typename std::conditional<V == 4, uint32_t, uint8_t>::type;
    const int lane = threadIdx.x & 63;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (scalar: the key reads and the predicate are too)
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    const bool no_infl = D.no_infl != 0;
    unsigned long long acc[MLM_DELTA_SUMS] = {};
    for (unsigned int s = blockIdx.x * (MLM_BLOCK / 64) + wave; s < D.nb; s += waves) {
        const int32_t *key = P.block_keys + 3 * (size_t)s;
        if (!mlm_age_selects(D.S, key[0], key[1], key[2])) { // (wave-uniform)
            if (lane == 0) D.packed[s] = MLM_WARP_EMPTY, D.slot_of[s] = s;
            continue;
        }
        const bool whole = P.explore && P.blk_collapsed[s]; // a released block: element 0 answers, infl 'u'
        unsigned long long d0 = 0, d1 = 0;
        bool full = false; // a voxel of this lane leaves the block non-empty
        if (whole) {
            const float L = P.log_odds[(size_t)s * C];
            const uint8_t o = P.occ[(size_t)s * C];
            const unsigned long long w = mlm_delta_word(mlm_fuse_bits(L), o, (uint8_t)'u');
            full = !mlm_age_voxel_empty(L, o, (uint8_t)'u');
            unsigned long long cg = ((unsigned long long)lane + 1ull) * MLM_DELTA_GOLD;
            for (size_t c = (size_t)lane; c < C; c += 64, cg += 64ull * MLM_DELTA_GOLD) mlm_delta_cell(cg, w, d0, d1);
        } else {
            const FT *la = (const FT *)(P.log_odds + (size_t)s * C);
            const BT *oa = (const BT *)(P.occ + (size_t)s * C), *ia = (const BT *)(P.infl + (size_t)s * C);
            unsigned long long cg = ((unsigned long long)lane * V + 1ull) * MLM_DELTA_GOLD; // of the trip's first voxel
            for (size_t i = (size_t)lane; i < C / V; i += 64, cg += (64ull * V) * MLM_DELTA_GOLD) {
                const FT va = la[i];
                const BT wa = oa[i], xa = ia[i];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float L = ((const float *)&va)[k];
                    const uint8_t o = (uint8_t)((uint32_t)wa >> (8 * k)), f = (uint8_t)((uint32_t)xa >> (8 * k));
                    full = full || !mlm_age_voxel_empty(L, o, f);
                    mlm_delta_cell(cg + (unsigned long long)k * MLM_DELTA_GOLD, mlm_delta_word(mlm_fuse_bits(L), o, no_infl ? (uint8_t)'u' : f), d0, d1);
                }
            }
        }
        // (wave-uniform from here: every lane meets the ballot and every shuffle)
        const bool empty = __ballot(full) == 0ull;
        for (int off = 32; off > 0; off >>= 1) d0 += __shfl_down(d0, off), d1 += __shfl_down(d1, off);
        if (lane == 0) {
            const int g[3] = {key[0], key[1], key[2]};
            D.packed[s] = mlm_warp_pack(g), D.slot_of[s] = s;
            D.dg[2 * (size_t)s] = d0, D.dg[2 * (size_t)s + 1] = d1;
            acc[MLM_DELTA_S_EMPTY] += empty;
            acc[MLM_DELTA_S_SELECTED] += 1;
        }
    }
    mlm_delta_part_row(acc, D.part + (size_t)blockIdx.x * MLM_DELTA_SUMS);
}

// items [0, nb): the sorted positions; items [nb, nb + n_prev): the rows of the previous table.  part: this kernel's rows.
__global__ __launch_bounds__(MLM_BLOCK) void k_delta_join(const MlmDelta D, unsigned long long *__restrict__ part, unsigned int *__restrict__ ctrl) {
    const unsigned int nb = D.nb, np = D.n_prev;
    const int32_t *const pk = D.prev_keys;
    const unsigned long long *const sorted = D.sorted;
    unsigned long long acc[MLM_DELTA_SUMS] = {};
    const unsigned long long items = (unsigned long long)nb + np;
    for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
        if (it < nb) {
            const unsigned int i = (unsigned int)it;
            const unsigned long long key = sorted[i];
            int kind = MLM_DELTA_K_NONE;
            if (key != MLM_WARP_EMPTY) {
                const uint32_t j = mlm_delta_lower_bound([&](uint32_t m) { return mlm_delta_pack3(pk + 3 * (size_t)m); }, np, key);
                const bool found = j < np && mlm_delta_pack3(pk + 3 * (size_t)j) == key;
                const size_t s = D.sorted_slot[i];
                const bool same = found && D.prev_dg[2 * (size_t)j] == D.dg[2 * s] && D.prev_dg[2 * (size_t)j + 1] == D.dg[2 * s + 1];
                kind = mlm_delta_kind(found, same);
                acc[MLM_DELTA_S_KIND + kind] += 1;
            }
            D.kind[i] = (uint32_t)kind;
        } else {
            const unsigned int j = (unsigned int)(it - nb);
            const int32_t *k = pk + 3 * (size_t)j;
            const unsigned long long key = mlm_delta_pack3(k);
            if (!mlm_delta_key_ok(k)) ctrl[2] = 1u;
            if (j + 1 < np && key >= mlm_delta_pack3(k + 3)) ctrl[3] = 1u;
            uint32_t st = MLM_DELTA_P_OUTSIDE;
            if (mlm_age_selects(D.S, k[0], k[1], k[2])) {
                const uint32_t i = mlm_delta_lower_bound([&](uint32_t m) { return sorted[m]; }, nb, key);
                const bool held = i < nb && sorted[i] == key;
                st = held ? MLM_DELTA_P_HELD : MLM_DELTA_P_GONE;
                acc[MLM_DELTA_S_INBOX] += 1;
                acc[MLM_DELTA_S_GONE] += !held;
            }
            D.pstate[j] = st;
        }
    }
    mlm_delta_part_row(acc, part + (size_t)blockIdx.x * MLM_DELTA_SUMS);
}

// the prefix over "state[i] is one of two values" of n items: counted per chunk, and — behind k_crop_scan — listed in ascending order
__global__ __launch_bounds__(MLM_BLOCK) void k_delta_count(const uint32_t *__restrict__ state, uint32_t a, uint32_t b, unsigned int n, unsigned int chunks,
                                                           unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_count_chunks([&](unsigned int i) { return state[i] == a || state[i] == b; }, n, chunks, chunk_cnt);
}
__global__ __launch_bounds__(MLM_BLOCK) void k_delta_rank(const uint32_t *__restrict__ state, uint32_t a, uint32_t b, unsigned int n, unsigned int chunks,
                                                          const unsigned int *__restrict__ chunk_cnt, unsigned int *__restrict__ list) {
    mlm_crop_rank_chunks([&](unsigned int i) { return state[i] == a || state[i] == b; }, n, chunks, chunk_cnt, [&](unsigned int i, unsigned int d, bool flagged) {
        if (flagged && d < n) list[d] = i; // (always: d counts flagged items below i)
    });
}

// table rows [0, S) — the first S sorted positions are the selected blocks — and gone keys [0, G); either pair of arrays may be null
__global__ __launch_bounds__(MLM_BLOCK) void k_delta_rows(const MlmDelta D, unsigned int S, unsigned int G, int32_t *__restrict__ cur_keys,
                                                          unsigned long long *__restrict__ cur_dg, int32_t *__restrict__ gone_keys) {
    const unsigned long long items = (unsigned long long)S + G;
    for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
        if (it < S) {
            const unsigned int i = (unsigned int)it;
            if (i >= D.nb) continue; // (never: S <= nb)
            if (cur_keys) {
                int g[3];
                mlm_warp_unpack(D.sorted[i], g);
                cur_keys[3 * (size_t)i] = g[0], cur_keys[3 * (size_t)i + 1] = g[1], cur_keys[3 * (size_t)i + 2] = g[2];
            }
            if (cur_dg) {
                const size_t s = D.sorted_slot[i];
                if (s < D.nb) cur_dg[2 * (size_t)i] = D.dg[2 * s], cur_dg[2 * (size_t)i + 1] = D.dg[2 * s + 1];
            }
        } else if (gone_keys) {
            const unsigned int r = (unsigned int)(it - S), j = D.glist[r];
            if (j >= D.n_prev) continue; // (never: see k_delta_rank)
#pragma unroll
            for (int a = 0; a < 3; ++a) gone_keys[3 * (size_t)r + a] = D.prev_keys[3 * (size_t)j + a];
        }
    }
}

// `bytes` at dst filled with a dword pattern by one wave, W bytes per lane and trip (dst W-byte aligned, bytes a multiple of W)
template <int W> __device__ __forceinline__ void mlm_delta_fill(void *__restrict__ dst, uint32_t pattern, size_t bytes, int lane) {
    using T = typename std::conditional<W == 16, uint4, typename std::conditional<W == 4, uint32_t, uint8_t>::type>::type;
    T v;
    if constexpr (W == 16) v = make_uint4(pattern, pattern, pattern, pattern);
    else v = (T)pattern;
    const size_t n = bytes / W;
    T *__restrict__ d = (T *)dst;
    for (size_t i = (size_t)lane; i < n; i += 64) d[i] = v;
}

// output rows [r0, r1): row r holds emitted block r, the block at sorted position elist[r]; the arrays start at row r0 (any may be null)
template <int FW, int BW>
__global__ __launch_bounds__(MLM_BLOCK) void k_delta_emit(const MlmDev P, const MlmDelta D, unsigned int r0, unsigned int r1, int32_t *__restrict__ keys,
                                                          float *__restrict__ lo, uint8_t *__restrict__ occ, uint8_t *__restrict__ infl,
                                                          uint8_t *__restrict__ kind) {
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    for (unsigned int r = r0 + blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); r < r1; r += waves) {
        const unsigned int i = D.elist[r];
        if (i >= D.nb) continue; // (never: see k_delta_rank)
        const unsigned int s = D.sorted_slot[i];
        if (s >= D.nb) continue; // (never: the sort's values are the slots)
        const size_t o = (size_t)(r - r0);
        if (keys && lane < 3) keys[3 * o + lane] = P.block_keys[3 * (size_t)s + lane];
        if (kind && lane == 3) kind[o] = (uint8_t)D.kind[i];
        const bool whole = P.explore && P.blk_collapsed[s];
        if (lo) {
            if (whole) mlm_delta_fill<FW>(lo + o * C, mlm_fuse_bits(P.log_odds[(size_t)s * C]), C * sizeof(float), lane);
            else mlm_crop_copy<FW>(lo + o * C, P.log_odds + (size_t)s * C, C * sizeof(float), lane);
        }
        if (occ) {
            if (whole) mlm_delta_fill<BW>(occ + o * C, (uint32_t)P.occ[(size_t)s * C] * 0x01010101u, C, lane);
            else mlm_crop_copy<BW>(occ + o * C, P.occ + (size_t)s * C, C, lane);
        }
        if (infl) {
            if (whole || D.no_infl) mlm_delta_fill<BW>(infl + o * C, (uint32_t)'u' * 0x01010101u, C, lane);
            else mlm_crop_copy<BW>(infl + o * C, P.infl + (size_t)s * C, C, lane);
        }
    }
}
