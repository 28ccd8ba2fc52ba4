// mlm_kernels_sweeps.h — batched segment casts for a ball of robot radius (mlm_query_sweeps; no reference counterpart: the reference has
// no segment query, so the classes are those of its point queries — what mlm_export_window's occ / infl channels return at a voxel —
// the path is mlm_raywalk.h's and the stop rule, the cap and the hit key are those of mlm_sweep.h, which the host mirror and the CPU
// test run too).
//
// k_sweeps0 (radius 0): one lane per ray, k_rays' form — mlm_ray_walk, then hit3 / hit_sq from its result.  A wave per ray would idle
// 63 lanes.
//
// k_sweeps (radius >= 1): one wave per ray, four rays per 256-thread workgroup, grid-stride over the rays.  The wave runs mlm_sweep_walk
// with wave-uniform state (the ray index goes through readfirstlane, so the DDA is scalar code).  The column table of the call's radius
// is built once per workgroup in LDS (<= 797 words; the only barrier).  Per step the 64 lanes stride over the L(r) columns of the cap,
// each forms its voxel from u_k's (block, cell) and an offset of at most 16 by compare-and-correct (no division by subbox_n), reads occ
// (and infl when INFL is selected), and one __ballot decides whether the step stops the ray — usually not, and then nothing else
// happens.  At a stop a 64-bit butterfly minimum of the key takes the winner (MlmNearScan::scan's reduction).  The start voxel's full
// ball is mlm_nearest.h's search under MlmNearScan.  Only the first lane stores.
//
// Block slots (CACHED): the block box that covers B(u_k) has at most kSweepNB blocks per axis when (2r - 1) / n + 2 <= kSweepNB (the
// host decides: n = 10 takes every radius, n = 5 radii up to 10).  Its slots live per wave in LDS on a torus — block g at
// (g mod kSweepNB) per axis, so a moving box never shifts its entries — filled once per ray by lanes probing in parallel, and when u_k
// crosses a block boundary only the entering layer (<= kSweepNB^2 blocks) is probed.  An entry is the slot, or -1 - class for an absent
// or a released block, which has one class for all its voxels and touches no plane memory.  Why every block of the box is fresh: take
// the last time one of its three indices entered the box's range; the other two were in range then (or theirs would be the last), the
// layer filled then holds it, and while it stays in the box nothing of the box shares its torus cell.  After every fill one ballot over
// the box's entries tells whether any block of it can hold a voxel with O at all; while none can (absent space under OCC, released FREE
// blocks) the cap is skipped and a step is the scalar DDA alone.  Larger boxes (small subbox_n
// with a large radius) take the other instantiation: one table probe per lane and voxel.
#pragma once
#include "mlm_kernels_nearest.h"
#include "mlm_kernels_rays.h"
#include "mlm_sweep.h"

constexpr int kSweepNB = 5; // blocks per axis of the cached box: 5^3 words per wave

struct MlmSweeps {
    const double *p0, *p1; // [n * 3]
    int n, radius, flags, cols; // cols = L(radius)
    int8_t *status;        // any output may be null
    int32_t *voxel3;
    double *t;
    int32_t *n_steps, *n_unknown, *hit3, *hit_sq;
};

__device__ __forceinline__ void mlm_sweeps_store(const MlmSweeps &R, int i, const MlmSweepResult &o) {
    if (R.status) R.status[i] = (int8_t)o.ray.status;
    if (R.voxel3) {
        R.voxel3[3 * (size_t)i] = o.ray.voxel[0];
        R.voxel3[3 * (size_t)i + 1] = o.ray.voxel[1];
        R.voxel3[3 * (size_t)i + 2] = o.ray.voxel[2];
    }
    if (R.t) R.t[i] = o.ray.t;
    if (R.n_steps) R.n_steps[i] = o.ray.n_steps;
    if (R.n_unknown) R.n_unknown[i] = o.ray.n_unknown;
    if (R.hit3) {
        R.hit3[3 * (size_t)i] = o.hit[0];
        R.hit3[3 * (size_t)i + 1] = o.hit[1];
        R.hit3[3 * (size_t)i + 2] = o.hit[2];
    }
    if (R.hit_sq) R.hit_sq[i] = o.hit_sq;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_sweeps0(const MlmDev P, const MlmSweeps R) {
    const int lanes = (int)(gridDim.x * blockDim.x);
    MlmRayClasses cls{P, -1, 4, true};
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < R.n; i += lanes) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = R.p0[3 * (size_t)i + k];
            b[k] = R.p1[3 * (size_t)i + k];
        }
        MlmSweepResult o;
        mlm_ray_walk(a, b, P.d_sub, P.n, R.flags, cls, o.ray);
        for (int k = 0; k < 3; ++k) o.hit[k] = o.ray.voxel[k]; // (the stop voxel itself, the end voxel, or 0 of an invalid ray)
        o.hit_sq = o.ray.status == 1 ? 0 : -1;
        mlm_sweeps_store(R, i, o);
    }
}

// mlm_sweep.h's callable, run by a whole wave with wave-uniform arguments
template <bool CACHED> struct MlmSweepVox {
    const MlmDev &P;
    const uint32_t *tab; // the column table (LDS)
    int cols;
    int *slots;          // this wave's kSweepNB^3 words (LDS)
    MlmNearScan near;
    int cslot, cfixed;   // the centre voxel's block
    bool cwhole;
    int glo[3], clo[3], ghi[3], chi[3]; // CACHED: block index and cell of u_k - r and of u_k + r
    bool live;           // CACHED: some block of the box can hold a voxel with O (as of the last layer that entered: conservative)

    __device__ __forceinline__ static int occ_bits(uint8_t r) { return r == 'o' ? 1 : (r == 'f' ? 0 : 4); }
    __device__ __forceinline__ static int tor(int g) {
        const int m = g % kSweepNB;
        return m < 0 ? m + kSweepNB : m;
    }
    __device__ __forceinline__ static int cell_of(int gx, int gy, int gz) { return (tor(gz) * kSweepNB + tor(gy)) * kSweepNB + tor(gx); }
    // the slot of a block with a class per voxel, else -1 - the class of all its voxels
    __device__ __forceinline__ int block_code(int gx, int gy, int gz) const {
        const int slot = mlm_block_find(P, gx, gy, gz);
        if (slot < 0) return -5;
        if (P.explore && P.blk_collapsed[slot]) return -1 - occ_bits(P.occ[(size_t)slot * P.cells]);
        return slot;
    }
    // the occ class of the path voxel (n_unknown): one probe per block crossed, one read per voxel
    __device__ __forceinline__ int centre(const int g[3], const int c[3], bool new_block) {
        if (new_block) {
            cslot = __builtin_amdgcn_readfirstlane(mlm_block_find(P, g[0], g[1], g[2]));
            cwhole = cslot < 0 || (P.explore && P.blk_collapsed[cslot]);
            cfixed = cslot < 0 ? 4 : (cwhole ? occ_bits(P.occ[(size_t)cslot * P.cells]) : 0);
        }
        if (cwhole) return cfixed;
        return occ_bits(P.occ[(size_t)cslot * P.cells + (size_t)((c[2] * P.n + c[1]) * P.n + c[0])]);
    }
    __device__ __forceinline__ void publish() const { // the wave's LDS writes before its reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // does any block of the box have a class per voxel, or one class that meets flags?  (wave-uniform)
    __device__ __forceinline__ bool box_live(int flags) const {
        bool any = false;
        for (int j = (int)(threadIdx.x & 63u); j < kSweepNB * kSweepNB * kSweepNB; j += 64) {
            const int jx = j % kSweepNB, jy = (j / kSweepNB) % kSweepNB, jz = j / (kSweepNB * kSweepNB);
            if (jx <= ghi[0] - glo[0] && jy <= ghi[1] - glo[1] && jz <= ghi[2] - glo[2]) {
                const int code = slots[cell_of(glo[0] + jx, glo[1] + jy, glo[2] + jz)];
                any = any || code >= 0 || ((-1 - code) & flags) != 0;
            }
        }
        return __ballot(any) != 0;
    }
    __device__ __forceinline__ unsigned long long start(const MlmRayState &S, int r, int flags) {
        const int n = P.n, lane = (int)(threadIdx.x & 63u);
        int u[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = S.g[a] * n + S.c[a];
        if (CACHED) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                glo[a] = ghi[a] = S.g[a];
                clo[a] = S.c[a] - r;
                chi[a] = S.c[a] + r;
                while (clo[a] < 0) clo[a] += n, --glo[a];
                while (chi[a] >= n) chi[a] -= n, ++ghi[a];
            }
            for (int j = lane; j < kSweepNB * kSweepNB * kSweepNB; j += 64) {
                const int jx = j % kSweepNB, jy = (j / kSweepNB) % kSweepNB, jz = j / (kSweepNB * kSweepNB);
                if (jx <= ghi[0] - glo[0] && jy <= ghi[1] - glo[1] && jz <= ghi[2] - glo[2])
                    slots[cell_of(glo[0] + jx, glo[1] + jy, glo[2] + jz)] = block_code(glo[0] + jx, glo[1] + jy, glo[2] + jz);
            }
            publish();
            live = box_live(flags);
            if (!live) return MLM_SWEEP_NOKEY; // (the ball lies inside the box)
        }
        return mlm_sweep_start(u, n, r, flags, near);
    }
    __device__ __forceinline__ unsigned long long cap(const MlmRayState &S, int axis, int s, bool, int, int flags) {
        const int n = P.n, lane = (int)(threadIdx.x & 63u);
        if (CACHED) {
            // the box moves one voxel along `axis`; a block layer enters when its leading face crosses a block boundary
            bool enter = false;
            int layer = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (a != axis) continue;
                clo[a] += s;
                chi[a] += s;
                if (s > 0) {
                    if (clo[a] >= n) clo[a] = 0, ++glo[a];
                    if (chi[a] >= n) chi[a] = 0, ++ghi[a], enter = true, layer = ghi[a];
                } else {
                    if (chi[a] < 0) chi[a] = n - 1, --ghi[a];
                    if (clo[a] < 0) clo[a] = n - 1, --glo[a], enter = true, layer = glo[a];
                }
            }
            if (enter) {
                // the two other axes b < c over their ranges, one block per lane
                const int lob = axis == 0 ? glo[1] : glo[0], hib = axis == 0 ? ghi[1] : ghi[0];
                const int loc = axis == 2 ? glo[1] : glo[2], hic = axis == 2 ? ghi[1] : ghi[2];
                const int jb = lane % kSweepNB, jc = lane / kSweepNB;
                if (lane < kSweepNB * kSweepNB && jb <= hib - lob && jc <= hic - loc) {
                    const int gb = lob + jb, gc = loc + jc;
                    const int gx = axis == 0 ? layer : gb, gy = axis == 1 ? layer : (axis == 0 ? gb : gc), gz = axis == 2 ? layer : gc;
                    slots[cell_of(gx, gy, gz)] = block_code(gx, gy, gz);
                }
                publish();
                live = box_live(flags);
            }
            if (!live) return MLM_SWEEP_NOKEY; // (absent space under OCC, free released blocks: the step is the DDA alone)
        }
        unsigned long long best = MLM_SWEEP_NOKEY;
        for (int base = 0; base < cols; base += 64) {
            const int j = base + lane;
            if (j < cols) {
                int off[3], g[3], c[3];
                const unsigned long long key = mlm_sweep_column_key(tab[j], axis, s, off);
#pragma unroll
                for (int a = 0; a < 3; ++a) { // |off| <= 16: compare and correct, no division by the runtime n
                    g[a] = S.g[a];
                    c[a] = S.c[a] + off[a];
                    while (c[a] < 0) c[a] += n, --g[a];
                    while (c[a] >= n) c[a] -= n, ++g[a];
                }
                const int code = CACHED ? slots[cell_of(g[0], g[1], g[2])] : block_code(g[0], g[1], g[2]);
                int bits;
                if (code < 0) {
                    bits = -1 - code;
                } else {
                    const size_t at = (size_t)code * P.cells + (size_t)((c[2] * n + c[1]) * n + c[0]);
                    bits = occ_bits(P.occ[at]);
                    if (flags & 2) bits |= P.infl[at] == 'o' ? 2 : 0;
                }
                if (bits & flags) best = key < best ? key : best;
            }
        }
        if (__ballot(best != MLM_SWEEP_NOKEY) == 0) return MLM_SWEEP_NOKEY; // (wave-uniform: the usual step)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { // butterfly minimum: every lane ends with the wave's
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), m);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other < best ? other : best;
        }
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)best);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(best >> 32));
        return ((unsigned long long)hi << 32) | lo;
    }
};

template <bool CACHED> __global__ __launch_bounds__(MLM_BLOCK) void k_sweeps(const MlmDev P, const MlmSweeps R) {
    __shared__ uint32_t s_tab[MLM_SWEEP_MAX_COLS];
    __shared__ int s_slots[MLM_BLOCK / 64][kSweepNB * kSweepNB * kSweepNB];
    // the column table: a thread per row
    if ((int)threadIdx.x <= 2 * R.radius) {
        const int q = (int)threadIdx.x - R.radius, w = mlm_sweep_row_half(R.radius, q);
        int at = mlm_sweep_row_begin(R.radius, q);
        for (int p = -w; p <= w; ++p) s_tab[at++] = mlm_sweep_column(R.radius, p, q);
    }
    __syncthreads();
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    MlmSweepVox<CACHED> vox{P, s_tab, R.cols, s_slots[threadIdx.x >> 6], MlmNearScan{P, -1}, -1, 4, true, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, true};
    for (int i = wave0; i < R.n; i += waves) {
        double a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = R.p0[3 * (size_t)i + k];
            b[k] = R.p1[3 * (size_t)i + k];
        }
        MlmSweepResult o;
        mlm_sweep_walk(a, b, P.d_sub, P.n, R.radius, R.flags, vox, o);
        if ((threadIdx.x & 63u) == 0) mlm_sweeps_store(R, i, o);
    }
}
