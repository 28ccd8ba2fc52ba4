// mlm_kernels_path.h — traced and shortened paths through a parent field (mlm_query_paths; no reference counterpart: the reference has
// neither a cost field nor a path query; the rule is mlm_path.h's, which the entry point's host branch and the CPU test run too).
//
// k_paths: one wave per goal, four goals per 256-thread workgroup; no LDS, no barriers, no atomics.  The
// wave runs mlm_path_goal with wave-uniform state:
//  - the trace is a pointer chase (one dependent byte load per move, the byte through readfirstlane, so the voxel, the counters and the
//    branch are scalar code).  Lane k & 63 keeps u_k in registers and every 64th move the wave stores 64 path voxels at once into the
//    wave's scratch slot: three int32 arrays of max_moves + 1 entries, box-relative coordinates (no linear index, no division);
//  - the shortening tests, per anchor, the candidates of the window in batches of 64 from the far end, one candidate and one
//    visibility walk per lane; __ballot collects the batch and its lowest set lane is the farthest visible voxel, so the answer is the
//    contract's maximum whatever the batch size, and word [6] is hi - j;
//  - the length sum, the table words and the way points are wave-uniform values that lane 0 stores with ordinary vector stores.
// Every loop is bounded by the arguments: max_moves moves, at most max_moves anchors of ceil(lookahead / 64) batches, a walk of at most
// 3 * lookahead steps; no byte of the field can make one spin, and every voxel is tested against the box before its byte is read.
// The scratch slot is the goal's: the entry point launches chunks of goals whose slots fit its scratch bound.
#pragma once
#include "mlm_path.h"

struct MlmPaths {
    MlmPathField F;
    int32_t lo[3];
    const int32_t *goals3; // [n * 3]
    int n, L, max_moves, cap;
    double d;              // (double)(float)subbox_d_xyz
    int32_t *scratch;      // [n][3][max_moves + 1]
    int8_t *status;        // any output may be null
    int32_t *way3;
    double *length;
    int64_t *table;
};

// mlm_path.h's executor for a whole wave
struct MlmPathWave {
    int32_t *px, *py, *pz; // the wave's slot
    int lane;
    int bx, by, bz;        // u_k of the last k with (k & 63) == lane
    __device__ __forceinline__ void put(int k, int x, int y, int z) {
        if ((k & 63) == lane) bx = x, by = y, bz = z;
        if ((k & 63) == 63) { // (wave-uniform) u_{k-63} .. u_k, one per lane
            const int at = k - 63 + lane;
            px[at] = bx, py[at] = by, pz[at] = bz;
        }
    }
    __device__ __forceinline__ void sync(int K) {
        if ((K & 63) != 63 && lane <= (K & 63)) { // the rest: u_{K & ~63} .. u_K
            const int at = (K & ~63) + lane;
            px[at] = bx, py[at] = by, pz[at] = bz;
        }
        __threadfence_block(); // the lanes read each other's stores below
    }
    __device__ __forceinline__ void at(int k, int v[3]) const { v[0] = px[k], v[1] = py[k], v[2] = pz[k]; }
    __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }
    __device__ __forceinline__ bool leader() const { return lane == 0; }
    __device__ __forceinline__ int pick(const MlmPathField &F, int i, int hi) const {
        int a[3];
        at(i, a);
        MLM_ROUTE_UNROLL
        for (int x = 0; x < 3; ++x) a[x] = uni(a[x]);
        for (int top = hi; top > i + 1; top -= 64) { // lane l tests j = top - l: lane 0 the farthest
            const int j = top - lane;
            bool ok = false;
            if (j > i + 1) {
                int b[3];
                at(j, b);
                ok = mlm_path_vis(F, a, b);
            }
            const unsigned long long m = __ballot(ok);
            if (m) return top - (int)__builtin_ctzll(m);
        }
        return i + 1;
    }
};

__global__ __launch_bounds__(MLM_BLOCK) void k_paths(const MlmPaths Q) {
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6))); // the wave's goal and slot
    if (i >= Q.n) return;
    const size_t len = (size_t)Q.max_moves + 1;
    int32_t *slot = Q.scratch + (size_t)i * 3 * len;
    MlmPathWave X{slot, slot + len, slot + 2 * len, (int)(threadIdx.x & 63u), 0, 0, 0};
    const int32_t goal[3] = {Q.goals3[3 * (size_t)i], Q.goals3[3 * (size_t)i + 1], Q.goals3[3 * (size_t)i + 2]};
    const MlmPathOut o{Q.status ? Q.status + i : nullptr, Q.way3 ? Q.way3 + 3 * (size_t)i * (size_t)Q.cap : nullptr,
                       Q.length ? Q.length + i : nullptr, Q.table ? Q.table + (size_t)i * MLM_PATH_WORDS : nullptr};
    mlm_path_goal(Q.F, Q.lo, goal, Q.L, Q.max_moves, Q.cap, Q.d, X, o);
}
