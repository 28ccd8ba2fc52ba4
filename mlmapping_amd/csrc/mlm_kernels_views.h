// mlm_kernels_views.h — distinct-voxel accounting of grouped ray fans (mlm_query_views; no reference counterpart: the reference has no
// view query).  The rules — bounding box, clipping, bit index, which counters a newly seen voxel bumps, which view takes which
// path — are mlm_views.h's, which the CPU test runs too; the walk is mlm_raywalk.h's, the classes MlmRayClasses'.
//
// k_views_box: per view the box spanned by the start and end voxels of its valid rays.  A workgroup takes up to kViewBoxRays rays
// of one view; a wave reduces its lanes' boxes by shuffles and issues one atomic per bound.
// k_views_lds: one workgroup per view, the view's bitset in LDS (launched per size class with that class's bytes).  A lane walks a
// ray at a time (stride: the workgroup); every voxel is one atomic OR on the LDS word, and only the lane that finds the bit clear
// reads the exclude byte, writes the mark byte and counts.  Counters: registers, then a shuffle reduction per wave, one LDS
// atomic per wave and counter, and the row written by plain stores.
// k_views_global: the same with the bitset in global scratch (cleared by the host driver's memset of the batch's words) and several
// workgroups per view; their counters meet in the zeroed table row by 64-bit atomic adds.
// No workgroup waits for another one.  mark: a voxel is a traversed voxel or a stop voxel for every ray of the call alike, so all
// lanes that write a byte write the same value into it (old | bit) and plain byte stores do.
#pragma once
#include "mlm_kernels_rays.h"
#include "mlm_views.h"

struct MlmViews {
    const double *p0, *p1;  // the chunk's rays [.. * 3]
    int flags;
    MlmViewWindow B;
    const uint8_t *exclude; // window layout of B, or null
    uint8_t *mark;          // the same
    const MlmViewBox *raw;  // per view of the chunk
    int64_t *table;         // [views of the chunk][kViewRow], or null
    uint32_t *scratch;      // bitsets of the global path's batch
};

__global__ __launch_bounds__(256) void k_views_box_init(MlmViewBox *raw, int n_views) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < n_views) mlm_view_box_reset(raw[k]);
}

__global__ __launch_bounds__(256) void k_views_box(const MlmDev P, const double *p0, const double *p1, const MlmViewJob *jobs, int n_jobs,
                                                    MlmViewBox *raw) {
    for (int j = (int)blockIdx.x; j < n_jobs; j += (int)gridDim.x) {
        const MlmViewJob J = jobs[j];
        MlmViewBox b;
        mlm_view_box_reset(b);
        for (int i = J.ray0 + (int)threadIdx.x; i < J.ray1; i += (int)blockDim.x) {
            double a[3], e[3];
            for (int k = 0; k < 3; ++k) {
                a[k] = p0[3 * (size_t)i + k];
                e[k] = p1[3 * (size_t)i + k];
            }
            MlmRayState S;
            if (mlm_ray_setup(a, e, P.d_sub, P.n, S)) mlm_view_box_add(b, S, P.n);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int lo = b.lo[a], hi = b.hi[a];
            for (int off = 32; off > 0; off >>= 1) {
                lo = min(lo, __shfl_down(lo, off, 64));
                hi = max(hi, __shfl_down(hi, off, 64));
            }
            if ((threadIdx.x & 63) == 0 && lo <= hi) {
                atomicMin(&raw[J.view].lo[a], lo);
                atomicMax(&raw[J.view].hi[a], hi);
            }
        }
    }
}

// what a lane has counted for the view it is walking
struct MlmViewCount {
    unsigned int trav, unknown, free_, stop, stopped, invalid;
    unsigned long long steps;
};

struct MlmViewVisit {
    const MlmViews &V;
    const MlmViewClip &C;
    uint32_t *bits;
    MlmViewCount &n;
    __device__ __forceinline__ void operator()(int vx, int vy, int vz, int cls, bool stop) {
        const int idx = mlm_view_bit(C, vx, vy, vz);
        if (idx < 0) return;
        const unsigned int m = 1u << (idx & 31);
        if (!mlm_view_new(atomicOr(&bits[idx >> 5], m), m)) return;
        bool excluded = false;
        if (V.B.on) { // (exclude and mark need the box)
            const size_t at = mlm_view_at(V.B, vx, vy, vz);
            if (V.exclude) excluded = V.exclude[at] != 0;
            if (V.mark) V.mark[at] |= mlm_view_mark_bits(stop);
        }
        mlm_view_account(cls, stop, excluded, n.trav, n.unknown, n.free_, n.stop);
    }
};

// rays ray0 + first, + stride, ... of a view into the bitset; then the workgroup's counters into s_cnt (LDS, zeroed, a barrier behind it)
__device__ __forceinline__ void mlm_views_walk(const MlmDev &P, const MlmViews &V, const MlmViewClip &C, uint32_t *bits, int ray0, int ray1, int first,
                                               int stride, unsigned long long *s_cnt) {
    MlmViewCount n{};
    MlmRayClasses cls{P, -1, 4, true};
    MlmViewVisit visit{V, C, bits, n};
    for (long long i = (long long)ray0 + first; i < ray1; i += stride) {
        double a[3], e[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = V.p0[3 * (size_t)i + k];
            e[k] = V.p1[3 * (size_t)i + k];
        }
        int k_steps;
        const int st = mlm_view_walk(a, e, P.d_sub, P.n, V.flags, cls, visit, k_steps);
        if (st < 0) {
            n.invalid += 1;
        } else {
            n.stopped += (unsigned int)st;
            n.steps += (unsigned long long)k_steps;
        }
    }
    unsigned long long w[7] = {n.trav, n.unknown, n.free_, n.stop, n.stopped, n.invalid, n.steps};
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        for (int off = 32; off > 0; off >>= 1) w[c] += __shfl_down(w[c], off, 64);
        if ((threadIdx.x & 63) == 0 && w[c]) atomicAdd(&s_cnt[c], w[c]);
    }
}

__global__ __launch_bounds__(kViewLdsThreads) void k_views_lds(const MlmDev P, const MlmViews V, const MlmViewJob *jobs, int n_jobs) {
    extern __shared__ uint32_t s_bits[];
    __shared__ unsigned long long s_cnt[kViewRow];
    for (int j = (int)blockIdx.x; j < n_jobs; j += (int)gridDim.x) {
        const MlmViewJob J = jobs[j];
        MlmViewClip C;
        mlm_view_clip(V.raw[J.view], V.B, C);
        const int words = (int)mlm_view_words(C.bits); // (the plan put the view into a class that holds them)
        for (int w = (int)threadIdx.x; w < words; w += (int)blockDim.x) s_bits[w] = 0u;
        if (threadIdx.x < kViewRow) s_cnt[threadIdx.x] = 0ull;
        __syncthreads();
        mlm_views_walk(P, V, C, s_bits, J.ray0, J.ray1, (int)threadIdx.x, (int)blockDim.x, s_cnt);
        __syncthreads();
        if (V.table && threadIdx.x < kViewRow) V.table[(size_t)J.view * kViewRow + threadIdx.x] = (int64_t)s_cnt[threadIdx.x]; // ([7] stays 0)
        __syncthreads();
    }
}

__global__ __launch_bounds__(kViewGlobalThreads) void k_views_global(const MlmDev P, const MlmViews V, const MlmViewJob *jobs, int n_jobs) {
    __shared__ unsigned long long s_cnt[kViewRow];
    for (int j = (int)blockIdx.x; j < n_jobs; j += (int)gridDim.x) {
        const MlmViewJob J = jobs[j];
        MlmViewClip C;
        mlm_view_clip(V.raw[J.view], V.B, C);
        if (threadIdx.x < kViewRow) s_cnt[threadIdx.x] = 0ull;
        __syncthreads();
        mlm_views_walk(P, V, C, V.scratch + J.word_off, J.ray0, J.ray1, J.part * (int)blockDim.x + (int)threadIdx.x, J.parts * (int)blockDim.x, s_cnt);
        __syncthreads();
        if (V.table && threadIdx.x < kViewRow - 1 && s_cnt[threadIdx.x])
            atomicAdd((unsigned long long *)&V.table[(size_t)J.view * kViewRow + threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads();
    }
}

// refused views: word [7] of their zeroed rows
__global__ __launch_bounds__(256) void k_views_refused(int64_t *table, const int *views, int n) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < n) table[(size_t)views[k] * kViewRow + kViewRow - 1] = 1;
}
