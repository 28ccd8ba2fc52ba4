// mlm_kernels_cluster.h — connected components of a voxel set of a box, with per-component statistics (mlm_export_clusters; no
// reference counterpart: the reference has no clustering, set, components and numbering are defined in include/mlmap_hip.h on the
// classes mlm_export_window reads out).
//
// The mask of the box (one byte per voxel) is k_esdf_mask's for the class sets; for the frontier k_cluster_occ reads the occ class
// of the box grown by one voxel per side (the same brick walk, one hash lookup per brick) and k_cluster_frontier combines a voxel
// with its six neighbours.  Then, on the union-find field of mlm_cluster.h (u32 per voxel), one launch each:
//  - k_cluster_local:   one workgroup per tile, labels in LDS, mlm_cluster_local_step until a pass changes nothing; stores the box
//                       index of each voxel's tile-local root and clears the voxel's size word;
//  - k_cluster_merge:   a lane per voxel; for every forward neighbour beyond the voxel's tile, mlm_cluster_union through atomicMin.
//                       Lock-free: a lane retries from the value its atomic returned, nobody waits for anybody;
//  - k_cluster_flatten: field[v] = root(v), and one atomicAdd per run of lanes with the same root on the root's size word;
//  - k_cluster_count / k_cluster_scan / k_cluster_rank: kept roots per chunk of kClusterChunk voxels, an exclusive scan of the
//                       chunk counts (one workgroup: at most 2^20 of them), the rank of each kept root = its component's number,
//                       stored over the size word (MLM_CLUSTER_OFF: dropped); the root starts its table row;
//  - k_cluster_write:   labels of a range of the box, and the rows: a segmented reduction over each run of lanes with the same
//                       label, then 64-bit integer atomics from the run's first lane, skipped where a look at the row shows that
//                       they cannot change it.
// Loads that may race with another lane's atomicMin or store (merge, flatten) are aligned 32-bit accesses, and every value such a
// load can return is a member of the same component that is not larger than the voxel (mlm_cluster.h), so a stale value costs a
// step, never the result.
#pragma once
#include "mlm_cluster.h"
#include "mlm_kernels_esdf.h"

struct MlmCluster {
    long long D[3];  // box dims
    long long lo[3]; // box origin (voxel indices)
    long long n[3];  // tiles per axis
    long long tiles, nvox;
    int T[3];        // tile dims (the last tile per axis is cut to the box)
    int nfwd;        // forward offsets of the connectivity
    uint32_t min_size;
    uint32_t *field; // [D2][D1][D0]
    uint32_t *num;   // sizes at the roots, then numbers
};

struct MlmClusterOcc {
    long long glo[3], gd[3]; // grown box: origin (voxel indices), dims
    long long b0[3];         // blocks covering it: first block index per axis ...
    int nb[3];               // ... and count
    uint8_t *out;            // [gd2][gd1][gd0]: occ class + 1 (0 UNKNOWN, 1 OCCUPIED, 2 FREE)
};

__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_occ(const MlmDev P, const MlmClusterOcc E) {
    __shared__ int s_slot;
    const long long n_bricks = (long long)E.nb[0] * E.nb[1] * E.nb[2];
    const int n = P.n;
    for (long long b = blockIdx.x; b < n_bricks; b += gridDim.x) {
        const int bx = (int)(b % E.nb[0]), by = (int)((b / E.nb[0]) % E.nb[1]), bz = (int)(b / ((long long)E.nb[0] * E.nb[1]));
        const long long gx = E.b0[0] + bx, gy = E.b0[1] + by, gz = E.b0[2] + bz;
        __syncthreads(); // (everyone has read the previous brick's slot)
        if (threadIdx.x == 0) s_slot = mlm_block_find(P, mlm_win_key(gx), mlm_win_key(gy), mlm_win_key(gz));
        __syncthreads();
        const int slot = s_slot;
        const bool collapsed = slot >= 0 && P.explore && P.blk_collapsed[slot];
        const long long x0 = max(gx * n, E.glo[0]), x1 = min(gx * n + n, E.glo[0] + E.gd[0]);
        const long long y0 = max(gy * n, E.glo[1]), y1 = min(gy * n + n, E.glo[1] + E.gd[1]);
        const long long z0 = max(gz * n, E.glo[2]), z1 = min(gz * n + n, E.glo[2] + E.gd[2]);
        const int ex = (int)(x1 - x0), ey = (int)(y1 - y0), ez = (int)(z1 - z0);
        const int nv = ex * ey * ez;
        const size_t base = (size_t)(slot >= 0 ? slot : 0) * P.cells;
        for (int j = threadIdx.x; j < nv; j += blockDim.x) {
            const int ix = j % ex, iy = (j / ex) % ey, iz = j / (ex * ey);
            const long long x = x0 + ix, y = y0 + iy, z = z0 + iz;
            const int cx = (int)(x - gx * n), cy = (int)(y - gy * n), cz = (int)(z - gz * n);
            const size_t at = base + (collapsed ? 0 : cz * n * n + cy * n + cx);
            E.out[((size_t)(z - E.glo[2]) * E.gd[1] + (size_t)(y - E.glo[1])) * E.gd[0] + (size_t)(x - E.glo[0])] =
                (uint8_t)(mlm_win_occ(P, slot, at) + 1);
        }
    }
}

// frontier: FREE with an UNKNOWN face neighbour; occ1: k_cluster_occ's array of the box grown by one voxel per side
__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_frontier(const uint8_t *__restrict__ occ1, uint8_t *__restrict__ mask, long long D0,
                                                                long long D1, long long nvox) {
    const size_t gy = (size_t)D0 + 2, gz = gy * (size_t)(D1 + 2);
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nvox; j += (long long)gridDim.x * blockDim.x) {
        const long long x = j % D0, y = (j / D0) % D1, z = j / (D0 * D1);
        const size_t g = (size_t)(z + 1) * gz + (size_t)(y + 1) * gy + (size_t)(x + 1);
        bool f = false;
        if (occ1[g] == 2)
            f = occ1[g - 1] == 0 || occ1[g + 1] == 0 || occ1[g - gy] == 0 || occ1[g + gy] == 0 || occ1[g - gz] == 0 || occ1[g + gz] == 0;
        mask[j] = (uint8_t)f;
    }
}

// cnt: [0] voxels of S, [1] components, [2] kept components, [3] voxels in them, [4] largest component, [5] most local passes of a
// tile that holds a voxel of S
__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_local(const MlmCluster R, const uint8_t *__restrict__ mask,
                                                             unsigned long long *__restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_cluster_dyn[];
    uint32_t *s = (uint32_t *)s_cluster_dyn; // [td2][td1][td0]
    unsigned most = 0;
    for (long long t = blockIdx.x; t < R.tiles; t += gridDim.x) {
        const long long t0 = t % R.n[0], t1 = (t / R.n[0]) % R.n[1], t2 = t / (R.n[0] * R.n[1]);
        const long long o[3] = {t0 * R.T[0], t1 * R.T[1], t2 * R.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)min((long long)R.T[a], R.D[a] - o[a]);
        const int nv = td[0] * td[1] * td[2], sz = td[0] * td[1];
        __syncthreads(); // (everyone is done with the previous tile)
        int any = 0;
        for (int i = threadIdx.x; i < nv; i += blockDim.x) {
            const int ix = i % td[0], iy = (i / td[0]) % td[1], iz = i / sz;
            const size_t g = ((size_t)(o[2] + iz) * R.D[1] + (size_t)(o[1] + iy)) * R.D[0] + (size_t)(o[0] + ix);
            const bool in = mask[g] != 0;
            s[i] = in ? (uint32_t)i : MLM_CLUSTER_OFF;
            any |= in;
        }
        unsigned passes = 0;
        if (__syncthreads_or(any)) {
            int more;
            do {
                int ch = 0;
                for (int i = threadIdx.x; i < nv; i += blockDim.x) {
                    const int ix = i % td[0], iy = (i / td[0]) % td[1], iz = i / sz;
                    const uint32_t v = s[i], w = mlm_cluster_local_step(s, ix, iy, iz, td, R.nfwd);
                    if (w != v) {
                        s[i] = w;
                        ch = 1;
                    }
                }
                more = __syncthreads_or(ch);
                ++passes;
            } while (more);
        }
        most = max(most, passes);
        for (int i = threadIdx.x; i < nv; i += blockDim.x) {
            const int ix = i % td[0], iy = (i / td[0]) % td[1], iz = i / sz;
            const size_t g = ((size_t)(o[2] + iz) * R.D[1] + (size_t)(o[1] + iy)) * R.D[0] + (size_t)(o[0] + ix);
            uint32_t r = s[i];
            if (r != MLM_CLUSTER_OFF) {
                const int rx = (int)(r % (uint32_t)td[0]), ry = (int)((r / (uint32_t)td[0]) % (uint32_t)td[1]), rz = (int)(r / (uint32_t)sz);
                r = (uint32_t)(((size_t)(o[2] + rz) * R.D[1] + (size_t)(o[1] + ry)) * R.D[0] + (size_t)(o[0] + rx));
            }
            R.field[g] = r;
            R.num[g] = 0;
        }
    }
    if (threadIdx.x == 0 && most) atomicMax(&cnt[5], (unsigned long long)most);
}

__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_merge(const MlmCluster R) {
    uint32_t *f = R.field;
    auto ld = [f](uint32_t i) { return __hip_atomic_load(&f[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto amin = [f](uint32_t i, uint32_t v) { return atomicMin(&f[i], v); };
    const long long sy = R.D[0], sz = R.D[0] * R.D[1];
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < R.nvox; j += (long long)gridDim.x * blockDim.x) {
        if (f[j] == MLM_CLUSTER_OFF) continue; // (an entry never becomes or ceases to be MLM_CLUSTER_OFF)
        const long long x = j % sy, y = (j / sy) % R.D[1], z = j / sz;
        const int ix = (int)(x % R.T[0]), iy = (int)(y % R.T[1]), iz = (int)(z % R.T[2]);
        for (int k = 0; k < R.nfwd; ++k) {
            int dx, dy, dz;
            mlm_cluster_fwd(k, dx, dy, dz);
            if (!mlm_cluster_leaves(ix, iy, iz, dx, dy, dz, R.T)) continue;
            const long long ux = x + dx, uy = y + dy, uz = z + dz;
            if (ux < 0 || ux >= R.D[0] || uy < 0 || uy >= R.D[1] || uz >= R.D[2]) continue; // (dz >= 0)
            const long long u = j + dx + dy * sy + dz * sz;
            if (f[u] == MLM_CLUSTER_OFF) continue;
            mlm_cluster_union(ld, amin, (uint32_t)j, (uint32_t)u);
        }
    }
}

// the lanes of a wave that start a run of equal keys (lane 0 and every lane whose key differs from the lane before), and the
// length of the run a starting lane starts
__device__ __forceinline__ unsigned long long mlm_cluster_run_heads(uint32_t key, int lane) {
    const uint32_t prev = __shfl_up(key, 1);
    return __ballot(lane == 0 || key != prev);
}
__device__ __forceinline__ int mlm_cluster_run_len(unsigned long long heads, int lane) {
    const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
    return rest ? __builtin_ctzll(rest) + 1 : 64 - lane;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_flatten(const MlmCluster R, unsigned long long *__restrict__ cnt) {
    __shared__ unsigned s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t *f = R.field;
    auto ld = [f](uint32_t i) { return f[i]; };
    const int lane = threadIdx.x & 63;
    unsigned n_s = 0;
    // (whole waves stay in the loop: the ballot sees every lane)
    for (long long b = (long long)blockIdx.x * blockDim.x; b < R.nvox; b += (long long)gridDim.x * blockDim.x) {
        const long long j = b + threadIdx.x;
        uint32_t root = MLM_CLUSTER_OFF;
        if (j < R.nvox && f[j] != MLM_CLUSTER_OFF) {
            root = mlm_cluster_find(ld, (uint32_t)j);
            f[j] = root;
        }
        const unsigned long long heads = mlm_cluster_run_heads(root, lane);
        if (((heads >> lane) & 1ull) && root != MLM_CLUSTER_OFF) {
            const unsigned run = (unsigned)mlm_cluster_run_len(heads, lane);
            atomicAdd(&R.num[root], run);
            n_s += run;
        }
    }
    if (n_s) atomicAdd(&s_n, n_s);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(&cnt[0], (unsigned long long)s_n);
}

// kept roots per chunk; components, voxels in kept components, the largest component
__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_count(const MlmCluster R, long long chunks, unsigned int *__restrict__ chunk_cnt,
                                                             unsigned long long *__restrict__ cnt) {
    __shared__ unsigned s_kept, s_big, s_roots;
    __shared__ unsigned long long s_vox;
    unsigned roots = 0, big = 0;
    unsigned long long kept_vox = 0;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        __syncthreads(); // (thread 0 has read the previous chunk's count)
        if (threadIdx.x == 0) s_kept = 0;
        __syncthreads();
        unsigned kept = 0;
        for (long long j = c * kClusterChunk + threadIdx.x; j < min(R.nvox, (c + 1) * kClusterChunk); j += blockDim.x) {
            if (R.field[j] != (uint32_t)j) continue;
            const uint32_t size = R.num[j];
            ++roots;
            big = max(big, size);
            if (size >= R.min_size) {
                ++kept;
                kept_vox += size;
            }
        }
        if (kept) atomicAdd(&s_kept, kept);
        __syncthreads();
        if (threadIdx.x == 0) chunk_cnt[c] = s_kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s_big = s_roots = 0;
        s_vox = 0;
    }
    __syncthreads();
    if (roots) {
        atomicAdd(&s_roots, roots);
        atomicMax(&s_big, big);
    }
    if (kept_vox) atomicAdd(&s_vox, kept_vox);
    __syncthreads();
    if (threadIdx.x == 0 && s_roots) {
        atomicAdd(&cnt[1], (unsigned long long)s_roots);
        atomicAdd(&cnt[3], s_vox);
        atomicMax(&cnt[4], (unsigned long long)s_big);
    }
}

// exclusive scan of the chunk counts in place, by one workgroup; the total is K
__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_scan(unsigned int *__restrict__ chunk_cnt, long long chunks,
                                                            unsigned long long *__restrict__ cnt) {
    __shared__ unsigned long long s_scan[MLM_BLOCK];
    unsigned long long carry = 0;
    for (long long b = 0; b < chunks; b += MLM_BLOCK) {
        const long long c = b + threadIdx.x;
        const unsigned v = c < chunks ? chunk_cnt[c] : 0u;
        __syncthreads(); // (the previous round's sums are read)
        s_scan[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < MLM_BLOCK; d <<= 1) {
            const unsigned long long add = threadIdx.x >= (unsigned)d ? s_scan[threadIdx.x - d] : 0ull;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < chunks) chunk_cnt[c] = (unsigned)(carry + s_scan[threadIdx.x] - v); // (K <= voxels < 2^31)
        carry += s_scan[MLM_BLOCK - 1];
    }
    if (threadIdx.x == 0) cnt[2] = carry;
}

// the number of every root over its size word; rows [0, cap) started by their roots
__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_rank(const MlmCluster R, long long chunks, const unsigned int *__restrict__ chunk_cnt,
                                                            int64_t *__restrict__ table, int cap) {
    __shared__ unsigned s_wave[MLM_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        unsigned base = chunk_cnt[c];
        // (whole workgroups stay in the loop: ballots and barriers see every lane)
        for (long long b = c * kClusterChunk; b < min(R.nvox, (c + 1) * kClusterChunk); b += blockDim.x) {
            const long long j = b + threadIdx.x;
            const bool root = j < R.nvox && R.field[j] == (uint32_t)j;
            const uint32_t size = root ? R.num[j] : 0u;
            const bool kept = root && size >= R.min_size;
            const unsigned long long bal = __ballot(kept);
            __syncthreads(); // (the previous round's wave totals are read)
            if (lane == 0) s_wave[wave] = (unsigned)__builtin_popcountll(bal);
            __syncthreads();
            unsigned before = 0, total = 0;
            for (int w = 0; w < MLM_BLOCK / 64; ++w) {
                if (w < wave) before += s_wave[w];
                total += s_wave[w];
            }
            if (root) {
                const unsigned k = base + before + (unsigned)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
                R.num[j] = kept ? k : MLM_CLUSTER_OFF;
                if (kept && k < (unsigned)cap) {
                    const long long r[3] = {j % R.D[0], (j / R.D[0]) % R.D[1], j / (R.D[0] * R.D[1])};
                    mlm_cluster_row_init(table + (size_t)k * MLM_CLUSTER_ROW_I64, size, r, R.lo);
                }
            }
            base += total;
        }
    }
}

// labels of the voxels [j0, j1) of the box (labels points at voxel j0; may be NULL) and what they add to the rows (table may be NULL)
__global__ __launch_bounds__(MLM_BLOCK) void k_cluster_write(const MlmCluster R, long long j0, long long j1, int32_t *__restrict__ labels,
                                                             int64_t *__restrict__ table, int cap) {
    const int lane = threadIdx.x & 63;
    auto add = [](int64_t *p, int64_t v) {
        if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // (a row entry only moves one way, so an older value than the current one can only make the look say "go on")
    auto amin = [](int64_t *p, int64_t v) {
        if (v < *(volatile int64_t *)p) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto amax = [](int64_t *p, int64_t v) {
        if (v > *(volatile int64_t *)p) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto aor = [](int64_t *p, int64_t v) {
        if (v & ~*(volatile int64_t *)p) __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // (whole waves stay in the loop: ballots and shuffles see every lane)
    for (long long b = j0 + (long long)blockIdx.x * blockDim.x; b < j1; b += (long long)gridDim.x * blockDim.x) {
        const long long j = b + threadIdx.x;
        int32_t lab = -1;
        if (j < j1) {
            const uint32_t root = R.field[j];
            lab = mlm_cluster_label(root, root == MLM_CLUSTER_OFF ? MLM_CLUSTER_OFF : R.num[root]);
            if (labels) labels[j - j0] = lab;
        }
        const bool row = table && j < j1 && lab >= 0 && lab < cap;
        if (!__ballot(row)) continue;
        const uint32_t key = row ? (uint32_t)lab : MLM_CLUSTER_OFF;
        const unsigned long long heads = mlm_cluster_run_heads(key, lane);
        const int left = mlm_cluster_run_len(heads | (1ull << lane), lane) - 1; // lanes after this one in its run
        const long long jj = row ? j : 0;
        const int x = (int)(jj % R.D[0]), y = (int)((jj / R.D[0]) % R.D[1]), z = (int)(jj / (R.D[0] * R.D[1]));
        int mn[3] = {x, y, z}, mx[3] = {x, y, z};
        long long sum[3] = {x, y, z};
        unsigned faces = mlm_cluster_faces(x, y, z, R.D);
        for (int d = 1; d < 64; d <<= 1) {
            const bool take = d <= left; // (lane + d lies in the same run, and holds the reduction of the run's next d lanes at most)
            for (int a = 0; a < 3; ++a) {
                const int omn = __shfl_down(mn[a], d), omx = __shfl_down(mx[a], d);
                const long long os = __shfl_down(sum[a], d);
                if (take) {
                    mn[a] = min(mn[a], omn);
                    mx[a] = max(mx[a], omx);
                    sum[a] += os;
                }
            }
            const unsigned of = __shfl_down(faces, d);
            if (take) faces |= of;
        }
        if (row && ((heads >> lane) & 1ull)) {
            const long long mn64[3] = {mn[0], mn[1], mn[2]}, mx64[3] = {mx[0], mx[1], mx[2]};
            mlm_cluster_row_update(table + (size_t)lab * MLM_CLUSTER_ROW_I64, mn64, mx64, sum, faces, R.lo, add, amin, amax, aor);
        }
    }
}
