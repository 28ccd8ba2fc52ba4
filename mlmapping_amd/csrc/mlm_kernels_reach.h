// mlm_kernels_reach.h — cost-to-go field through the free space of a voxel box (mlm_export_reach; no reference counterpart: the
// reference has no such field, it is defined in include/mlmap_hip.h on the classes mlm_export_window reads out).
//
// The blocked mask of the box (one byte per voxel) comes from the ESDF's kernels: clearance 0, k_esdf_mask on the box itself (the
// window's brick walk, one hash lookup per brick); clearance r > 0, the ESDF tile passes at C = r + 1 (mlm_kernels_esdf.h) and
// k_reach_blocked, which thresholds D_out <= r^2.  Then, on the working field of mlm_reach.h (u32 per voxel):
//  - k_reach_init:  MLM_REACH_BLOCKED / MLM_REACH_FAR from the mask; k_reach_seed: 0 at the effective seeds, their tiles (and, for a seed on a
//                   tile face, the tile beyond it) dirty;
//  - k_reach_sweep: one workgroup per DIRTY tile: the tile and a one-voxel halo staged in LDS, relaxed there until a whole pass
//                   changes nothing, the lowered voxels written back, and for every face with a lowered voxel the tile beyond it
//                   marked dirty in the NEXT sweep's array (and the sweep's "marked" word bumped, which is what the host reads);
//  - k_reach_out:   steps, parent and the summary counters of a range of the box.
// No workgroup waits for another: a tile that read a halo its neighbour lowered in the same sweep is marked by that neighbour
// and runs again in the next one (values only decrease towards the least fixpoint, mlm_reach.h), so the launch boundary is the
// only ordering.  Halo loads and write-backs of one sweep may therefore overlap in time; both are aligned 32-bit accesses, and
// either value a load returns is the length of a real path.
#pragma once
#include "mlm_kernels_esdf.h"
#include "mlm_reach.h"

struct MlmReach {
    long long D[3];  // box dims
    long long n[3];  // tiles per axis
    long long tiles;
    int T[3];        // tile dims (the last tile per axis is cut to the box)
    uint32_t max_steps;
    uint32_t *field; // [D2][D1][D0]
};

// blocked = D_out <= r2, for the contiguous range of the box that one ESDF tile covers (field: the tile's D_out, same order)
__global__ __launch_bounds__(MLM_BLOCK) void k_reach_blocked(const uint16_t *__restrict__ field, uint8_t *__restrict__ mask, long long nt,
                                                             unsigned r2) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (long long)gridDim.x * blockDim.x)
        mask[j] = (uint8_t)(field[j] <= r2);
}

__global__ __launch_bounds__(MLM_BLOCK) void k_reach_init(const uint8_t *__restrict__ mask, uint32_t *__restrict__ field, long long nvox) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nvox; j += (long long)gridDim.x * blockDim.x)
        field[j] = mask[j] ? MLM_REACH_BLOCKED : MLM_REACH_FAR;
}

// seeds: absolute voxel index triples; one outside the box or on a blocked voxel contributes nothing
__global__ __launch_bounds__(MLM_BLOCK) void k_reach_seed(const MlmReach R, const int32_t *__restrict__ seeds, int n_seeds, long long lo0,
                                                          long long lo1, long long lo2, uint8_t *__restrict__ dirty) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seeds; i += gridDim.x * blockDim.x) {
        const long long x = seeds[3 * i] - lo0, y = seeds[3 * i + 1] - lo1, z = seeds[3 * i + 2] - lo2;
        if (x < 0 || x >= R.D[0] || y < 0 || y >= R.D[1] || z < 0 || z >= R.D[2]) continue;
        const size_t at = ((size_t)z * R.D[1] + (size_t)y) * R.D[0] + (size_t)x;
        if (R.field[at] == MLM_REACH_BLOCKED) continue; // (other lanes only ever store 0 here)
        R.field[at] = 0u;
        // a seed is a lowered voxel: its own tile is dirty, and so are the tiles beyond the faces it lies on
        const long long t[3] = {x / R.T[0], y / R.T[1], z / R.T[2]};
        const long long in[3] = {x - t[0] * R.T[0], y - t[1] * R.T[1], z - t[2] * R.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)min((long long)R.T[a], R.D[a] - t[a] * R.T[a]);
        dirty[(t[2] * R.n[1] + t[1]) * R.n[0] + t[0]] = 1;
        const unsigned faces = mlm_reach_faces((int)in[0], (int)in[1], (int)in[2], td);
        for (int c = 0; c < 6; ++c) {
            const long long nt = ((faces >> c) & 1u) ? mlm_reach_tile_beyond(t[0], t[1], t[2], R.n, c) : -1;
            if (nt >= 0) dirty[nt] = 1;
        }
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_reach_sweep(const MlmReach R, uint8_t *__restrict__ cur, uint8_t *__restrict__ next,
                                                           unsigned int *__restrict__ marked) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_reach_dyn[];
    uint32_t *s = (uint32_t *)s_reach_dyn; // [td2 + 2][td1 + 2][td0 + 2]
    __shared__ unsigned s_dirty, s_faces;
    for (long long t = blockIdx.x; t < R.tiles; t += gridDim.x) {
        __syncthreads(); // (everyone is done with the previous tile)
        if (threadIdx.x == 0) {
            s_dirty = cur[t];
            s_faces = 0;
            cur[t] = 0; // (this array is the next sweep's `next`: it must be clear by then, and only this workgroup reads the entry)
        }
        __syncthreads();
        if (!s_dirty) continue;
        const long long t0 = t % R.n[0], t1 = (t / R.n[0]) % R.n[1], t2 = t / (R.n[0] * R.n[1]);
        const long long o[3] = {t0 * R.T[0], t1 * R.T[1], t2 * R.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)min((long long)R.T[a], R.D[a] - o[a]);
        const int sy = td[0] + 2, sz = sy * (td[1] + 2), hv = sz * (td[2] + 2);
        for (int i = threadIdx.x; i < hv; i += blockDim.x) {
            const int hx = i % sy, hy = (i / sy) % (td[1] + 2), hz = i / sz;
            const long long gx = o[0] + hx - 1, gy = o[1] + hy - 1, gz = o[2] + hz - 1;
            const bool in = gx >= 0 && gx < R.D[0] && gy >= 0 && gy < R.D[1] && gz >= 0 && gz < R.D[2];
            s[i] = in ? R.field[((size_t)gz * R.D[1] + (size_t)gy) * R.D[0] + (size_t)gx] : MLM_REACH_BLOCKED;
        }
        __syncthreads();
        // relax in place, a column of z per lane, down and up again; a pass without a store ends it (a lane may read a value another
        // lane stores in the same pass: older or newer, both are path lengths)
        const int cols = td[0] * td[1];
        int more;
        do {
            int ch = 0;
            for (int col = threadIdx.x; col < cols; col += blockDim.x) {
                const int ix = col % td[0], iy = col / td[0];
                int c = sz + (iy + 1) * sy + ix + 1;
                for (int iz = 0; iz < td[2]; ++iz, c += sz) {
                    const uint32_t v = s[c], w = mlm_reach_relax(v, s[c - 1], s[c + 1], s[c - sy], s[c + sy], s[c - sz], s[c + sz], R.max_steps);
                    if (w != v) {
                        s[c] = w;
                        ch = 1;
                    }
                }
                for (int iz = td[2] - 2; iz >= 0; --iz) {
                    c -= sz;
                    const int d = c - sz;
                    const uint32_t v = s[d], w = mlm_reach_relax(v, s[d - 1], s[d + 1], s[d - sy], s[d + sy], s[d - sz], s[d + sz], R.max_steps);
                    if (w != v) {
                        s[d] = w;
                        ch = 1;
                    }
                }
            }
            more = __syncthreads_or(ch);
        } while (more);
        // write the lowered voxels back; the faces they lie on
        unsigned faces = 0;
        for (int col = threadIdx.x; col < cols; col += blockDim.x) {
            const int ix = col % td[0], iy = col / td[0];
            int c = sz + (iy + 1) * sy + ix + 1;
            size_t g = ((size_t)o[2] * R.D[1] + (size_t)(o[1] + iy)) * R.D[0] + (size_t)(o[0] + ix);
            for (int iz = 0; iz < td[2]; ++iz, c += sz, g += (size_t)R.D[0] * R.D[1]) {
                const uint32_t v = s[c];
                if (v < R.field[g]) { // (only this workgroup stores to its tile)
                    R.field[g] = v;
                    faces |= mlm_reach_faces(ix, iy, iz, td);
                }
            }
        }
        if (faces) atomicOr(&s_faces, faces);
        __syncthreads();
        if (threadIdx.x < 6 && ((s_faces >> threadIdx.x) & 1u)) {
            const long long nt = mlm_reach_tile_beyond(t0, t1, t2, R.n, (int)threadIdx.x);
            if (nt >= 0) {
                next[nt] = 1;
                atomicAdd(marked, 1u);
            }
        }
    }
}

// steps / parent of the voxels [j0, j1) of the box (outputs point at voxel j0; either may be NULL) and the summary counters:
// cnt[0] traversable, cnt[1] reached, cnt[2] largest steps + 1 (0: none)
__global__ __launch_bounds__(MLM_BLOCK) void k_reach_out(const MlmReach R, long long j0, long long j1, int32_t *__restrict__ steps,
                                                         uint8_t *__restrict__ parent, unsigned long long *__restrict__ cnt) {
    __shared__ unsigned s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned n_trav = 0, n_reached = 0, top = 0;
    const long long sy = R.D[0], sz = R.D[0] * R.D[1];
    for (long long j = j0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += (long long)gridDim.x * blockDim.x) {
        const uint32_t v = R.field[j];
        if (steps) steps[j - j0] = mlm_reach_steps(v);
        n_trav += v != MLM_REACH_BLOCKED;
        if (v < MLM_REACH_FAR) {
            ++n_reached;
            top = max(top, v + 1u);
        }
        if (parent) {
            uint8_t p = 255;
            if (v < MLM_REACH_FAR) {
                const long long x = j % sy, y = (j / sy) % R.D[1], z = j / sz;
                const uint32_t nb[6] = {x > 0 ? R.field[j - 1] : MLM_REACH_BLOCKED,         x < R.D[0] - 1 ? R.field[j + 1] : MLM_REACH_BLOCKED,
                                        y > 0 ? R.field[j - sy] : MLM_REACH_BLOCKED,        y < R.D[1] - 1 ? R.field[j + sy] : MLM_REACH_BLOCKED,
                                        z > 0 ? R.field[j - sz] : MLM_REACH_BLOCKED,        z < R.D[2] - 1 ? R.field[j + sz] : MLM_REACH_BLOCKED};
                p = mlm_reach_parent(v, nb);
            }
            parent[j - j0] = p;
        }
    }
    if (n_trav) atomicAdd(&s_cnt[0], n_trav);
    if (n_reached) atomicAdd(&s_cnt[1], n_reached);
    if (top) atomicMax(&s_cnt[2], top);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(&cnt[0], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt[1], (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicMax(&cnt[2], (unsigned long long)s_cnt[2]);
    }
}
