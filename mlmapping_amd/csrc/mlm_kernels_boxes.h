// mlm_kernels_boxes.h — class counts and free-space growth of axis-aligned voxel boxes (mlm_query_boxes; no reference counterpart:
// the reference has no volume query, so the classes are those of its point queries — what mlm_export_window's occ / infl channels
// return at a voxel — and the growth is the round and face loop of mlm_boxgrow.h, which the host mirror and the CPU test run too).
//
// k_boxes: one wave per item, four items per 256-thread workgroup, grid-stride over the items; no LDS, no barriers.  The wave runs
// mlm_box_grow with wave-uniform state (the item index goes through readfirstlane, so the box, the limits and the counters sit in
// scalar registers); the only per-lane work is the scan of a box or slab: the 64 lanes stride over its voxels in x-fastest order,
// each lane steps its (x, y, z) by the mixed-radix digits of 64 (no division per voxel beyond the split into block and cell), and
// the wave decides with two ballots per step — one for "has O", one for UNKNOWN — whose population counts are the counters.  A
// rejected slab returns at the first step that saw O; the blocked start counts on.  A lane keeps the slot of the block its last
// voxel was in and probes the block table again only when its next voxel lies in another block; an absent or a released block has
// one class for all its voxels and touches no plane memory.  Every voxel of the final box is read once, plus at most six rejected
// slabs.  (One workgroup per item and an LDS copy of the limit region were not built: DESIGN.md.)
#pragma once
#include "mlm_boxgrow.h"
#include "mlm_kernels_window.h"

struct MlmBoxes {
    const int32_t *box6; // [n * 6]
    int n, flags;
    MlmBoxLimits lim;
    int8_t *status;      // any output may be null
    int32_t *out6;
    uint8_t *closed;
    int64_t *table;      // [n * MLM_BOX_ROW]
};

// mlm_boxgrow.h's callable, run by a whole wave
struct MlmBoxScan {
    const MlmDev &P;
    int g[3];        // the block of the lane's last voxel ...
    int slot, fixed; // ... its slot, and the class of every voxel of an absent (UNKNOWN) or released (element 0, inflated class UNKNOWN) block
    bool whole;
    __device__ __forceinline__ static int occ_bits(uint8_t r) { return r == 'o' ? 1 : (r == 'f' ? 0 : 4); }
    // classes of the voxel (gl * n + t): t >= 0 per axis, the offset from the first cell of block gl
    __device__ __forceinline__ int classes(const int gl[3], uint32_t tx, uint32_t ty, uint32_t tz) {
        const uint32_t n = (uint32_t)P.n;
        const uint32_t qx = tx / n, qy = ty / n, qz = tz / n;
        const int gx = gl[0] + (int)qx, gy = gl[1] + (int)qy, gz = gl[2] + (int)qz;
        if (gx != g[0] || gy != g[1] || gz != g[2]) {
            g[0] = gx, g[1] = gy, g[2] = gz;
            slot = mlm_block_find(P, gx, gy, gz);
            whole = slot < 0 || (P.explore && P.blk_collapsed[slot]);
            fixed = slot < 0 ? 4 : (whole ? occ_bits(P.occ[(size_t)slot * P.cells]) : 0);
        }
        if (whole) return fixed;
        const uint32_t cx = tx - qx * n, cy = ty - qy * n, cz = tz - qz * n;
        const size_t at = (size_t)slot * P.cells + (size_t)((cz * n + cy) * n + cx);
        return occ_bits(P.occ[at]) | (P.infl[at] == 'o' ? 2 : 0);
    }
    __device__ __forceinline__ void operator()(const int32_t lo[3], const int32_t hi[3], int flags, bool full, long long &n_unknown,
                                               long long &n_obstacle) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t n = (uint32_t)P.n;
        int gl[3];
        uint32_t cl[3], e[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { // the block of the box's first voxel and that voxel's cell: floor division without leaving 32 bits (lo may be INT_MIN)
            const int v = lo[a];
            const int q = v >= 0 ? (int)((uint32_t)v / n) : -(int)((uint32_t)(-(v + 1)) / n) - 1;
            gl[a] = q;
            cl[a] = (uint32_t)v - (uint32_t)q * n; // (modulo 2^32: q * n may lie below INT_MIN, the difference is in [0, n))
            e[a] = (uint32_t)hi[a] - (uint32_t)v + 1u;
        }
        // layers of z in chunks of fewer than 2^31 voxels (a plane has fewer than 2^31), so that the flat index fits 32 bits
        const uint32_t plane = e[0] * e[1];
        const uint32_t zc = 0x7FFFFFFFu / plane;
        // the digits of one step of 64 voxels
        const uint32_t dx = 64u % e[0], t64 = 64u / e[0], dy = t64 % e[1], dz = t64 / e[1];
        for (uint32_t z0 = 0; z0 < e[2]; z0 += zc) {
            const uint32_t nz = min(zc, e[2] - z0), total = plane * nz;
            uint32_t x = lane % e[0], t = lane / e[0], y = t % e[1], z = z0 + t / e[1];
            for (uint32_t base = 0; base < total; base += 64u) {
                const bool act = base + lane < total;
                int bits = 0;
                if (act) bits = classes(gl, cl[0] + x, cl[1] + y, cl[2] + z);
                const unsigned long long m_o = __ballot(act && (bits & flags) != 0), m_u = __ballot(act && (bits & 4) != 0);
                n_obstacle += __popcll(m_o);
                n_unknown += __popcll(m_u);
                if (!full && m_o) return; // (wave-uniform)
                x += dx;
                if (x >= e[0]) {
                    x -= e[0];
                    ++y;
                }
                y += dy;
                if (y >= e[1]) {
                    y -= e[1];
                    ++z;
                }
                z += dz;
            }
        }
    }
};

__global__ __launch_bounds__(MLM_BLOCK) void k_boxes(const MlmDev P, const MlmBoxes B) {
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    MlmBoxScan scan{P, {(int)0x80000000, 0, 0}, -1, 4, true};
    for (int i = wave0; i < B.n; i += waves) {
        int32_t b6[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) b6[k] = B.box6[6 * (size_t)i + k];
        MlmBoxResult o;
        mlm_box_grow(b6, B.flags, B.lim, scan, o);
        if ((threadIdx.x & 63u) == 0) {
            if (B.status) B.status[i] = (int8_t)o.status;
            if (B.out6)
#pragma unroll
                for (int k = 0; k < 6; ++k) B.out6[6 * (size_t)i + k] = o.box[k];
            if (B.closed) B.closed[i] = (uint8_t)o.closed;
            if (B.table)
#pragma unroll
                for (int k = 0; k < 4; ++k) B.table[4 * (size_t)i + k] = o.row[k];
        }
    }
}
