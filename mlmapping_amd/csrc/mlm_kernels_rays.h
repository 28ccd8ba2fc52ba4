// mlm_kernels_rays.h — batched segment casts through the voxel map (mlm_query_rays; no reference counterpart: the reference has
// no segment query, so the classes are those of its point queries — what mlm_export_window's occ / infl channels return at a
// voxel — and the path is the integer walk of mlm_raywalk.h, which the host mirror and the CPU test run too).
//
// k_rays: one lane per ray.  A lane keeps the slot of the block it is in and probes the block table again only when the walk
// crosses into another block; an absent or a released block has one class for all its voxels, so the steps inside it touch no
// memory.  The walk's state is 18 32-bit values per lane, the only wide arithmetic the two 64-bit products of a comparison; no LDS.
//
// Rays of one batch differ in length by orders of magnitude and stop early.  The loop is the plain grid-stride one with the walk
// inside, at most four rays per lane in a launch of 2^20.  A flattened form — one loop in which a lane that has finished its ray
// sets its next one up while its neighbours keep stepping — was built and measured on the two batches of tools/ray_rate.py
// and was slower (edges 0.80 ms against 0.68 ms, views 1.05 ms against 0.79 ms: ten more registers and a loop body whose
// set-up branch every step has to jump over cost more than the idle lanes of a round), so it is not kept.
#pragma once
#include "mlm_kernels_window.h"
#include "mlm_raywalk.h"

struct MlmRays {
    const double *p0, *p1; // [n * 3]
    int n, flags;
    int8_t *status;        // any output may be null
    int32_t *voxel3;
    double *t;
    int32_t *n_steps, *n_unknown;
};

// the classes of the voxels of the block the ray is in (mlm_raywalk.h's callable)
struct MlmRayClasses {
    const MlmDev &P;
    int slot, fixed; // fixed: the class of every voxel of an absent (UNKNOWN) or released (element 0, inflated class UNKNOWN) block
    bool whole;
    __device__ __forceinline__ static int occ_bits(uint8_t r) { return r == 'o' ? 1 : (r == 'f' ? 0 : 4); }
    __device__ __forceinline__ int operator()(const int g[3], const int c[3], bool new_block) {
        if (new_block) {
            slot = mlm_block_find(P, g[0], g[1], g[2]);
            whole = slot < 0 || (P.explore && P.blk_collapsed[slot]);
            fixed = slot < 0 ? 4 : (whole ? occ_bits(P.occ[(size_t)slot * P.cells]) : 0);
        }
        if (whole) return fixed;
        const size_t at = (size_t)slot * P.cells + (size_t)((c[2] * P.n + c[1]) * P.n + c[0]);
        return occ_bits(P.occ[at]) | (P.infl[at] == 'o' ? 2 : 0);
    }
};

__device__ __forceinline__ void mlm_rays_store(const MlmRays &R, int i, const MlmRayResult &o) {
    if (R.status) R.status[i] = (int8_t)o.status;
    if (R.voxel3) {
        R.voxel3[3 * (size_t)i] = o.voxel[0];
        R.voxel3[3 * (size_t)i + 1] = o.voxel[1];
        R.voxel3[3 * (size_t)i + 2] = o.voxel[2];
    }
    if (R.t) R.t[i] = o.t;
    if (R.n_steps) R.n_steps[i] = o.n_steps;
    if (R.n_unknown) R.n_unknown[i] = o.n_unknown;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_rays(const MlmDev P, const MlmRays R) {
    const int lanes = (int)(gridDim.x * blockDim.x);
    MlmRayClasses cls{P, -1, 4, true};
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < R.n; i += lanes) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = R.p0[3 * (size_t)i + k];
            b[k] = R.p1[3 * (size_t)i + k];
        }
        MlmRayResult o;
        mlm_ray_walk(a, b, P.d_sub, P.n, R.flags, cls, o);
        mlm_rays_store(R, i, o);
    }
}
