// mlm_kernels_clearance.h — batched segment casts through a distance field (mlm_query_clearance; no reference counterpart: the
// reference has no segment query and no distance field.  The path is the integer walk of mlm_raywalk.h, the rule that of
// mlm_clearance.h, which the host branch and the CPU test run too).
//
// k_clearance<K>: one lane per ray, in k_rays' plain grid-stride form (mlm_kernels_rays.h records that a flattened refill loop was
// measured slower; it is not rebuilt here).  The kernel reads no map state: the field's box is kernel-argument data, the walk's state
// 18 32-bit values per lane plus the place in the field (three 64-bit coordinates and the index).  Unlike k_rays every voxel costs a
// load, and the path does not depend on what is read: K > 1 steps the walk K voxels ahead and has their K loads in flight together
// before the first is tested (mlm_clear_walk<K>; the entry parameters and voxels of the K stay in registers).  K = 1 and K = 4 are
// built; the knob "clear_ahead" chooses, DESIGN.md has the measurement.
//
// k_clearance_groups: one lane per group, a sequential scan of its segments' five words in the batch's scratch (mlm_clear_group).
#pragma once
#include "mlm_kernels.h"
#include "mlm_clearance.h"

struct MlmClear {
    const double *p0, *p1; // [n * 3]
    int n;
    double d;              // subbox_d_xyz
    MlmClearField F;
    int8_t *status;        // any output may be null
    int32_t *voxel3;
    double *t;
    int32_t *n_steps, *min_sq, *min3;
    int64_t *cost;
    int32_t *n_near;
    // the words the group rows need, for the rays of this launch (null without groups)
    int8_t *g_status;
    int32_t *g_min_sq, *g_steps, *g_near;
    int64_t *g_cost;
};

struct MlmClearGroups {
    const int32_t *begin; // [n_groups + 1]
    int n_groups;
    const int8_t *status; // the scratch of the whole batch
    const int32_t *min_sq, *n_steps, *n_near;
    const int64_t *cost;
    int64_t *table;       // [n_groups][MLM_CLEAR_WORDS]
};

__device__ __forceinline__ void mlm_clear_store(const MlmClear &R, int i, const MlmClearResult &o) {
    if (R.status) R.status[i] = (int8_t)o.status;
    if (R.voxel3) {
        R.voxel3[3 * (size_t)i] = o.voxel[0];
        R.voxel3[3 * (size_t)i + 1] = o.voxel[1];
        R.voxel3[3 * (size_t)i + 2] = o.voxel[2];
    }
    if (R.t) R.t[i] = o.t;
    if (R.n_steps) R.n_steps[i] = o.n_steps;
    if (R.min_sq) R.min_sq[i] = o.min_sq;
    if (R.min3) {
        R.min3[3 * (size_t)i] = o.min3[0];
        R.min3[3 * (size_t)i + 1] = o.min3[1];
        R.min3[3 * (size_t)i + 2] = o.min3[2];
    }
    if (R.cost) R.cost[i] = (int64_t)o.cost;
    if (R.n_near) R.n_near[i] = o.n_near;
    if (R.g_status) {
        R.g_status[i] = (int8_t)o.status;
        R.g_min_sq[i] = o.min_sq;
        R.g_steps[i] = o.n_steps;
        R.g_near[i] = o.n_near;
        R.g_cost[i] = (int64_t)o.cost;
    }
}

template <int K> __global__ __launch_bounds__(MLM_BLOCK) void k_clearance(const MlmClear R) {
    const int lanes = (int)(gridDim.x * blockDim.x);
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < R.n; i += lanes) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = R.p0[3 * (size_t)i + k];
            b[k] = R.p1[3 * (size_t)i + k];
        }
        MlmClearResult o;
        mlm_clear_walk<K>(a, b, R.d, R.F, o);
        mlm_clear_store(R, i, o);
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_clearance_groups(const MlmClearGroups G) {
    const int lanes = (int)(gridDim.x * blockDim.x);
    for (int g = (int)(blockIdx.x * blockDim.x + threadIdx.x); g < G.n_groups; g += lanes) {
        int64_t row[MLM_CLEAR_WORDS];
        mlm_clear_group(G.begin[g], G.begin[g + 1], G.status, G.min_sq, G.cost, G.n_steps, G.n_near, row);
        for (int w = 0; w < MLM_CLEAR_WORDS; ++w) G.table[(size_t)g * MLM_CLEAR_WORDS + w] = row[w];
    }
}
