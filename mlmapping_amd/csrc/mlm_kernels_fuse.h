// mlm_kernels_fuse.h — the kernels of mlm_fuse_blocks (include/mlmap_hip.h; the rule: mlm_fuse.h).  Part of mlmap_hip.hip.
//
//  - k_fuse_probe: a wave per row.  Lane 0 checks the key's range and looks the block up (mlm_block_find); the lanes stream the row's
//    occ (and infl) bytes — a dword per lane where the rows are 4-byte aligned, else a byte — and ballot the touch flag.  It writes the
//    row's slot (-1: absent), its flags and its packed key, and reads nothing of the map's planes.
//  - k_fuse_dups: the packed keys sorted by the host (mlm_sort_pairs_u64_u32), neighbours compared.
//  - k_fuse_count / k_crop_scan / k_fuse_rank: the rows that create a block numbered by mlm_kernels_crop.h's atomic-free three-phase
//    prefix: row r of rank d takes slot nb + d.  The host reads {created, range flag, duplicate flag} once and grows the pool if needed;
//    slots are pool indices and survive that.
//  - k_fuse_create: a lane per created row writes block_keys and inserts the key into the table with the slot it already has, as
//    k_rehash_blocks does.  A fresh slot's planes are 0 / 'u' / 'u' (alloc_pool, crop_reset_tail).
//  - k_fuse_apply<V, DRY>: a wave per row, V voxels per lane and trip (V = 4: one 16-byte load of La and of Lb, a dword each of occ_a,
//    occ_b, infl_a, infl_b; V = 1: the narrow path of subbox_n 3 and 7 and of unaligned sources).  mlm_fuse.h's rule, only what changed
//    is stored.  The counts are summed per lane, reduced per wave for per_row, kept in the lane across rows, reduced per workgroup
//    at the end and written as one row of twelve partial sums; k_fuse_sums adds the rows up — integer adds, one value whatever the
//    order, and no atomic.  DRY removes every store into the map, reads 0 / 'u' / 'u' for an absent block and element 0 / infl 'u'
//    for a released one (k_merge_pack's view).
#pragma once
#include "mlm_fuse.h"
#include "mlm_kernels_crop.h"

#define MLM_FUSE_CTRL_WORDS 4 // ctrl[0] = created rows (k_crop_scan), ctrl[1] = a key out of range, ctrl[2] = a duplicate key

struct MlmFuse {
    MlmFuseRule R;
    unsigned int n, nb;        // rows; blocks in use before the call
    const int32_t *keys;       // [n][3]
    const float *lo;           // [n][cells]
    const uint8_t *occ, *infl; // [n][cells]; infl may be null
    int32_t *row_slot;         // [n] slot of the row's block, -1: absent
    uint32_t *row_flag;        // [n] MLM_FUSE_R_*
    int32_t *row_new;          // [n] slot a created row takes, else -1
    int32_t *per_row;          // [n][4] or null
    unsigned long long *part;  // [workgroups of k_fuse_apply][12] partial sums
};

template <int V>
__global__ __launch_bounds__(MLM_BLOCK) void k_fuse_probe(const MlmDev P, const MlmFuse F, unsigned long long *__restrict__ packed, uint32_t *__restrict__ vals,
                                                          unsigned int *__restrict__ ctrl) {
    using T = typename std::conditional<V == 4, uint32_t, uint8_t>::type;
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    const bool has_infl = F.infl != nullptr;
    for (unsigned int r = blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); r < F.n; r += waves) {
        int slot = -1;
        uint32_t flags = 0;
        if (lane == 0) {
            const int32_t kx = F.keys[3 * (size_t)r], ky = F.keys[3 * (size_t)r + 1], kz = F.keys[3 * (size_t)r + 2];
            if (!mlm_fuse_key_ok(kx, ky, kz)) {
                flags |= MLM_FUSE_R_RANGE;
                ctrl[1] = 1u;
            } else {
                slot = mlm_block_find(P, kx, ky, kz);
                if (slot >= P.max_blocks) slot = -1; // (never: a slot of the table is a pool index)
            }
            packed[r] = mlm_fuse_pack(kx, ky, kz);
            vals[r] = r;
        }
        const T *__restrict__ ob = (const T *)(F.occ + (size_t)r * C);
        const T *__restrict__ ib = has_infl ? (const T *)(F.infl + (size_t)r * C) : nullptr;
        bool touch = false;
        for (size_t i = (size_t)lane; i < C / V; i += 64) {
            const T o = ob[i], f = has_infl ? ib[i] : (T)0;
            if (V == 4) touch = touch || mlm_fuse_touches4((uint32_t)o, has_infl, (uint32_t)f);
            else touch = touch || mlm_fuse_touches((uint8_t)o, has_infl, (uint8_t)f);
        }
        if (__ballot(touch) != 0ull) flags |= MLM_FUSE_R_TOUCH;
        if (lane == 0) {
            F.row_slot[r] = slot;
            F.row_flag[r] = flags;
        }
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_fuse_dups(const unsigned long long *__restrict__ sorted, unsigned int n, unsigned int *__restrict__ ctrl) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += gridDim.x * blockDim.x)
        if (sorted[i] == sorted[i + 1]) ctrl[2] = 1u;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_fuse_count(const MlmFuse F, unsigned int chunks, unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_count_chunks([&](unsigned int r) { return mlm_fuse_creates(F.row_slot[r], F.row_flag[r]); }, F.n, chunks, chunk_cnt);
}
__global__ __launch_bounds__(MLM_BLOCK) void k_fuse_rank(const MlmFuse F, unsigned int chunks, const unsigned int *__restrict__ chunk_cnt) {
    mlm_crop_rank_chunks([&](unsigned int r) { return mlm_fuse_creates(F.row_slot[r], F.row_flag[r]); }, F.n, chunks, chunk_cnt,
                         [&](unsigned int r, unsigned int d, bool creates) { F.row_new[r] = creates ? (int32_t)(F.nb + d) : -1; });
}

__global__ __launch_bounds__(MLM_BLOCK) void k_fuse_create(const MlmDev P, const MlmFuse F, unsigned int created) {
    if (blockIdx.x == 0 && threadIdx.x == 0) P.g->n_blocks = F.nb + created;
    for (unsigned int r = blockIdx.x * blockDim.x + threadIdx.x; r < F.n; r += gridDim.x * blockDim.x) {
        const int32_t s = F.row_new[r];
        if (s < (int32_t)F.nb || s >= P.max_blocks) continue; // (not a created row; beyond the pool: never, the host made room)
        const int32_t kx = F.keys[3 * (size_t)r], ky = F.keys[3 * (size_t)r + 1], kz = F.keys[3 * (size_t)r + 2];
        P.block_keys[3 * (size_t)s] = kx, P.block_keys[3 * (size_t)s + 1] = ky, P.block_keys[3 * (size_t)s + 2] = kz;
        const unsigned long long key = mlm_pack_key(kx, ky, kz);
        uint32_t at = mlm_mix(key) & P.ht_mask;
        for (uint32_t probe = 0; probe <= P.ht_mask; ++probe) {
            if (atomicCAS(&P.ht_keys[at], MLM_HT_EMPTY, key) == MLM_HT_EMPTY) {
                P.ht_slot[at] = s;
                break;
            }
            at = (at + 1) & P.ht_mask;
        }
    }
}

__device__ __forceinline__ uint32_t mlm_fuse_wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v; // (lane 0 holds the sum)
}

template <int V, bool DRY> __global__ __launch_bounds__(MLM_BLOCK) void k_fuse_apply(const MlmDev P, const MlmFuse F) {
    using FT = typename std::conditional<V == 4, float4, float>::type;
    using BT = typename std::conditional<V == 4, uint32_t, uint8_t>::type;
    const int lane = threadIdx.x & 63;
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const size_t C = (size_t)P.cells;
    const MlmFuseRule R = F.R;
    const bool has_infl = R.has_infl != 0;
    unsigned long long acc[MLM_FUSE_SUMS] = {};
    for (unsigned int r = blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6); r < F.n; r += waves) {
        const int32_t found = F.row_slot[r];
        const uint32_t flags = F.row_flag[r];
        const int32_t state = mlm_fuse_row_state(found, flags);
        int32_t slot = found >= 0 ? found : (DRY ? -1 : F.row_new[r]);
        if (slot >= P.max_blocks) slot = -1; // (never)
        uint32_t cnt[8] = {};
        // a row that touches nothing changes nothing and counts nothing; a created row without a slot: never
        if ((flags & MLM_FUSE_R_TOUCH) && !(flags & MLM_FUSE_R_RANGE) && (DRY || slot >= 0)) {
            bool whole = false;
            if (DRY) whole = slot >= 0 && P.explore && P.blk_collapsed[slot];
            const size_t base = (size_t)(slot >= 0 ? slot : 0) * C;
            const FT *__restrict__ lb = (const FT *)(F.lo + (size_t)r * C);
            const BT *__restrict__ ob = (const BT *)(F.occ + (size_t)r * C);
            const BT *__restrict__ ib = has_infl ? (const BT *)(F.infl + (size_t)r * C) : nullptr;
            FT *la = (FT *)(P.log_odds + base);
            BT *oa = (BT *)(P.occ + base), *ia = (BT *)(P.infl + base);
            for (size_t i = (size_t)lane; i < C / V; i += 64) {
                float La[V], Lb[V];
                uint8_t o_a[V], i_a[V], o_b[V], i_b[V];
                const FT vb = lb[i];
                const BT wb = ob[i], xb = has_infl ? ib[i] : (BT)0;
                FT va;
                BT wa, xa;
                if (DRY && slot < 0) {
                    __builtin_memset(&va, 0, sizeof(va));
                    wa = xa = (BT)(V == 4 ? 0x75757575u : 0x75u); // 'u'
                } else if (DRY && whole) {
                    const float L0 = P.log_odds[base];
                    const uint8_t o0 = P.occ[base];
                    for (int k = 0; k < V; ++k) ((float *)&va)[k] = L0;
                    wa = (BT)(V == 4 ? 0x01010101u * o0 : o0);
                    xa = (BT)(V == 4 ? 0x75757575u : 0x75u);
                } else {
                    va = la[i], wa = oa[i], xa = ia[i];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    La[k] = ((const float *)&va)[k], Lb[k] = ((const float *)&vb)[k];
                    o_a[k] = (uint8_t)((uint32_t)wa >> (8 * k)), i_a[k] = (uint8_t)((uint32_t)xa >> (8 * k));
                    o_b[k] = (uint8_t)((uint32_t)wb >> (8 * k)), i_b[k] = (uint8_t)((uint32_t)xb >> (8 * k));
                }
                uint32_t any = 0;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const uint32_t ev = mlm_fuse_voxel(R, La[k], o_a[k], i_a[k], Lb[k], o_b[k], i_b[k]);
                    any |= ev;
#pragma unroll
                    for (int b = 0; b < 8; ++b) cnt[b] += (ev >> b) & 1u;
                }
                if (!DRY) {
                    if (any & MLM_FUSE_E_LO) {
                        FT out;
#pragma unroll
                        for (int k = 0; k < V; ++k) ((float *)&out)[k] = La[k];
                        la[i] = out;
                    }
                    if (any & MLM_FUSE_E_OCC) {
                        uint32_t w = 0;
#pragma unroll
                        for (int k = 0; k < V; ++k) w |= (uint32_t)o_a[k] << (8 * k);
                        oa[i] = (BT)w;
                    }
                    if (any & MLM_FUSE_E_INFL) {
                        uint32_t w = 0;
#pragma unroll
                        for (int k = 0; k < V; ++k) w |= (uint32_t)i_a[k] << (8 * k);
                        ia[i] = (BT)w;
                    }
                }
            }
        }
        // (wave-uniform from here: every lane meets every shuffle)
        const uint32_t contrib = mlm_fuse_wave_sum(cnt[0]), conflict = mlm_fuse_wave_sum(cnt[3]), turned = mlm_fuse_wave_sum(cnt[4] + cnt[5]);
        if (lane == 0) {
            if (F.per_row) { // (a caller's array need not be 16-byte aligned)
                int32_t *const pr = F.per_row + MLM_FUSE_PR * (size_t)r;
                pr[0] = (int32_t)contrib, pr[1] = (int32_t)conflict, pr[2] = (int32_t)turned, pr[3] = state;
            }
            acc[1] += state == MLM_FUSE_ROW_PRESENT;
            acc[3] += !(flags & MLM_FUSE_R_TOUCH);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[4 + b] += cnt[b];
    }
    // per wave (shuffles), per workgroup (LDS), then one row of partial sums per workgroup — plain stores; k_fuse_sums adds the rows up
    // (every wave adding its own counts to the call's twelve words met on one cache line: 1.2 ms of a call over 16 384 rows)
    __shared__ unsigned long long s_part[MLM_BLOCK / 64][MLM_FUSE_SUMS];
#pragma unroll
    for (int k = 0; k < MLM_FUSE_SUMS; ++k) {
        unsigned long long v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) s_part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < MLM_FUSE_SUMS) {
        unsigned long long t = 0;
        for (int w = 0; w < MLM_BLOCK / 64; ++w) t += s_part[w][threadIdx.x];
        F.part[(size_t)blockIdx.x * MLM_FUSE_SUMS + threadIdx.x] = t;
    }
}

// the call's twelve sums from the workgroups' partial rows, by one workgroup: integer adds, one value whatever the order
__global__ __launch_bounds__(MLM_BLOCK) void k_fuse_sums(const unsigned long long *__restrict__ part, unsigned int rows, unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long s_part[MLM_BLOCK / 64][MLM_FUSE_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long acc[MLM_FUSE_SUMS] = {};
    for (unsigned int r = threadIdx.x; r < rows; r += MLM_BLOCK)
#pragma unroll
        for (int k = 0; k < MLM_FUSE_SUMS; ++k) acc[k] += part[(size_t)r * MLM_FUSE_SUMS + k];
#pragma unroll
    for (int k = 0; k < MLM_FUSE_SUMS; ++k) {
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off);
        if (lane == 0) s_part[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < MLM_FUSE_SUMS) {
        unsigned long long t = 0;
        for (int w = 0; w < MLM_BLOCK / 64; ++w) t += s_part[w][threadIdx.x];
        sums[threadIdx.x] = t;
    }
}
