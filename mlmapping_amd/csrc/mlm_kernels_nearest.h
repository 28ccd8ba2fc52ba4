// mlm_kernels_nearest.h — the exact nearest obstacle voxel of batched points (mlm_query_nearest; no reference counterpart: the reference
// has no such query, so the classes are those of its point queries — what mlm_export_window's occ / infl channels return at a voxel —
// and the metric, the tie rule and the search are those of mlm_nearest.h, which the host mirror and the CPU test run too).
//
// k_nearest: one wave per point, four points per 256-thread workgroup, grid-stride over the points; no LDS, no barriers, no atomics.
// The wave runs mlm_near_search with wave-uniform state (the point index goes through readfirstlane, so Q, v, the ring state, the
// bounds and the best key sit in scalar registers and the loop over rings and blocks is scalar code): one probe of the block table per
// block that the bounds let through, none per voxel.  The only per-lane work is the scan of one block: the 64 lanes stride over its
// cells inside the cube in x-fastest order, each lane steps its (x, y, z) by the mixed-radix digits of 64 (MlmBoxScan's stepping: no
// division per voxel), reads occ (and infl when INFL is selected), keeps the smallest key of its voxels with O inside the ball, and a
// 64-bit butterfly minimum over the wave makes the block's answer uniform — skipped when no lane found a candidate.  An absent or a
// released block touches no plane memory (mlm_nearest.h).  (A per-block "has an obstacle" summary would skip most scans; it would
// have to be kept by the integrate kernels: DESIGN.md.)
#pragma once
#include "mlm_kernels_window.h"
#include "mlm_nearest.h"

struct MlmNearest {
    const double *pos; // [n * 3]
    int n, C, flags;
    int8_t *status;    // any output may be null
    int32_t *voxel3, *delta3;
    int64_t *sq;
    double *dist;
};

// mlm_nearest.h's callable, run by a whole wave with wave-uniform arguments
struct MlmNearScan {
    const MlmDev &P;
    int slot;
    __device__ __forceinline__ static int occ_bits(uint8_t r) { return r == 'o' ? 1 : (r == 'f' ? 0 : 4); }
    __device__ __forceinline__ int probe(const int g[3]) {
        slot = __builtin_amdgcn_readfirstlane(mlm_block_find(P, g[0], g[1], g[2]));
        if (slot < 0) return 4;
        if (P.explore && P.blk_collapsed[slot]) return occ_bits(P.occ[(size_t)slot * P.cells]);
        return -1;
    }
    __device__ __forceinline__ unsigned long long scan(const MlmNearPoint &p, const int g[3], const int c0[3], const int c1[3], int flags) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t n = (uint32_t)P.n;
        const uint32_t e0 = (uint32_t)(c1[0] - c0[0] + 1), e1 = (uint32_t)(c1[1] - c0[1] + 1), e2 = (uint32_t)(c1[2] - c0[2] + 1);
        const uint32_t total = e0 * e1 * e2; // <= n^3
        // the digits of one step of 64 cells
        const uint32_t dx = 64u % e0, t64 = 64u / e0, dy = t64 % e1, dz = t64 / e1;
        uint32_t x = lane % e0, t = lane / e0, y = t % e1, z = t / e1;
        const uint8_t *occ = P.occ + (size_t)slot * P.cells, *infl = P.infl + (size_t)slot * P.cells;
        const int32_t ox = g[0] * (int)n + c0[0], oy = g[1] * (int)n + c0[1], oz = g[2] * (int)n + c0[2]; // the first voxel of the part
        unsigned long long best = MLM_NEAR_NOKEY;
        for (uint32_t base = 0; base < total; base += 64u) {
            if (base + lane < total) { // (then x < e0, y < e1, z < e2: the cell lies inside the block)
                const uint32_t at = (((uint32_t)c0[2] + z) * n + (uint32_t)c0[1] + y) * n + (uint32_t)c0[0] + x;
                int bits = occ_bits(occ[at]);
                if (flags & 2) bits |= infl[at] == 'o' ? 2 : 0;
                if (bits & flags) {
                    const int32_t o[3] = {ox + (int32_t)x, oy + (int32_t)y, oz + (int32_t)z};
                    const unsigned long long key = mlm_near_voxel_key(p, o);
                    best = key < best ? key : best;
                }
            }
            x += dx;
            if (x >= e0) {
                x -= e0;
                ++y;
            }
            y += dy;
            if (y >= e1) {
                y -= e1;
                ++z;
            }
            z += dz;
        }
        if (__ballot(best != MLM_NEAR_NOKEY) == 0) return MLM_NEAR_NOKEY; // (wave-uniform)
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

__global__ __launch_bounds__(MLM_BLOCK) void k_nearest(const MlmDev P, const MlmNearest Q) {
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    MlmNearScan vox{P, -1};
    for (int i = wave0; i < Q.n; i += waves) {
        double pos[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pos[a] = Q.pos[3 * (size_t)i + a];
        MlmNearResult o;
        mlm_near_search(pos, P.d_sub, P.n, Q.C, Q.flags, vox, o);
        if ((threadIdx.x & 63u) == 0) {
            if (Q.status) Q.status[i] = (int8_t)o.status;
            if (Q.voxel3)
#pragma unroll
                for (int a = 0; a < 3; ++a) Q.voxel3[3 * (size_t)i + a] = o.voxel[a];
            if (Q.delta3)
#pragma unroll
                for (int a = 0; a < 3; ++a) Q.delta3[3 * (size_t)i + a] = o.delta[a];
            if (Q.sq) Q.sq[i] = o.sq;
            if (Q.dist) Q.dist[i] = o.dist;
        }
    }
}
