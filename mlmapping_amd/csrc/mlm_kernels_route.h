// mlm_kernels_route.h — clearance-weighted cost field with face, edge and corner moves through the free space of a voxel box
// (mlm_export_route; no reference counterpart: the reference has no such field, it is defined in include/mlmap_hip.h on the classes
// mlm_export_window reads out and on mlm_export_esdf's D_out).
//
// The class byte of every voxel of the box (its ring, 255: blocked) comes from the ESDF's kernels: clearance 0 and no penalty,
// k_esdf_mask on the box itself (0 / 1: k_route_init reads "above n_penalty" as blocked, which holds for both forms); otherwise the
// ESDF tile passes at C = clearance + n_penalty + 1 (mlm_kernels_esdf.h) and k_route_class.  Then, on the working field of
// mlm_route.h (u32 per voxel):
//  - k_route_init:  MLM_REACH_BLOCKED / MLM_REACH_FAR from the class bytes; k_route_seed: 0 at the effective seeds, their tiles and
//                   the tiles whose halo holds them dirty;
//  - k_route_sweep: one workgroup per DIRTY tile: the tile and its full one-voxel halo (edges and corners too) staged in LDS, the
//                   entry penalty of every voxel of the tile beside it, relaxed there until a whole pass changes nothing, the
//                   lowered voxels written back, and every neighbouring tile whose halo holds a lowered voxel marked dirty in the
//                   NEXT sweep's array (and the sweep's "marked" word bumped, which is what the host reads); specialised on the
//                   connectivity, so that the 6-connected field does not pay for twenty neighbours it never takes;
//  - k_route_out:   cost, parent and the summary counters of a range of the box.
// As in mlm_kernels_reach.h no workgroup waits for another: the launch boundary is the only ordering, halo loads and write-backs
// of one sweep may overlap in time, both are aligned 32-bit accesses, and either value a load returns is the cost of a real path.
#pragma once
#include "mlm_kernels_esdf.h"
#include "mlm_route.h"

struct MlmRoute {
    long long D[3]; // box dims
    long long n[3]; // tiles per axis
    long long tiles;
    int T[3];       // tile dims (the last tile per axis is cut to the box)
    int connectivity;
    uint32_t max_cost;
    uint32_t move_cost[3];
    uint32_t *field;       // [D2][D1][D0]
    const uint8_t *cls;    // class byte per voxel, same layout
    const uint32_t *pen;   // 64 words: penalty[0 .. n_penalty - 1], then zeros
};

// class bytes of the contiguous range of the box that one ESDF tile covers (field: the tile's D_out, same order)
__global__ __launch_bounds__(MLM_BLOCK) void k_route_class(const uint16_t *__restrict__ field, uint8_t *__restrict__ cls, long long nt, int r,
                                                           int n_penalty) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (long long)gridDim.x * blockDim.x)
        cls[j] = mlm_route_class(field[j], r, n_penalty);
}

__global__ __launch_bounds__(MLM_BLOCK) void k_route_init(const uint8_t *__restrict__ cls, uint32_t *__restrict__ field, long long nvox,
                                                          int n_penalty) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nvox; j += (long long)gridDim.x * blockDim.x)
        field[j] = (int)cls[j] > n_penalty ? MLM_REACH_BLOCKED : MLM_REACH_FAR;
}

// seeds: absolute voxel index triples; one outside the box or on a blocked voxel contributes nothing
__global__ __launch_bounds__(MLM_BLOCK) void k_route_seed(const MlmRoute R, const int32_t *__restrict__ seeds, int n_seeds, long long lo0,
                                                          long long lo1, long long lo2, uint8_t *__restrict__ dirty) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seeds; i += gridDim.x * blockDim.x) {
        const long long x = seeds[3 * i] - lo0, y = seeds[3 * i + 1] - lo1, z = seeds[3 * i + 2] - lo2;
        if (x < 0 || x >= R.D[0] || y < 0 || y >= R.D[1] || z < 0 || z >= R.D[2]) continue;
        const size_t at = ((size_t)z * R.D[1] + (size_t)y) * R.D[0] + (size_t)x;
        if (R.field[at] == MLM_REACH_BLOCKED) continue; // (other lanes only ever store 0 here)
        R.field[at] = 0u;
        // a seed is a lowered voxel: its own tile is dirty, and so is every tile whose halo holds it
        const long long t[3] = {x / R.T[0], y / R.T[1], z / R.T[2]};
        const long long in[3] = {x - t[0] * R.T[0], y - t[1] * R.T[1], z - t[2] * R.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)min((long long)R.T[a], R.D[a] - t[a] * R.T[a]);
        dirty[(t[2] * R.n[1] + t[1]) * R.n[0] + t[0]] = 1;
        const uint32_t m = mlm_route_dirty_mask(mlm_reach_faces((int)in[0], (int)in[1], (int)in[2], td), R.connectivity);
        for (int k = 0; k < 27; ++k) {
            const long long nt = ((m >> k) & 1u) ? mlm_route_tile_at(t[0], t[1], t[2], R.n, k) : -1;
            if (nt >= 0) dirty[nt] = 1;
        }
    }
}

template <int CONN>
__global__ __launch_bounds__(MLM_BLOCK) void k_route_sweep(const MlmRoute R, uint8_t *__restrict__ cur, uint8_t *__restrict__ next,
                                                           unsigned int *__restrict__ marked) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_route_dyn[];
    uint32_t *s = (uint32_t *)s_route_dyn; // [td2 + 2][td1 + 2][td0 + 2], then the tile's entry penalties u16 [td2][td1][td0]
    __shared__ unsigned s_dirty, s_mask;
    for (long long t = blockIdx.x; t < R.tiles; t += gridDim.x) {
        __syncthreads(); // (everyone is done with the previous tile)
        if (threadIdx.x == 0) {
            s_dirty = cur[t];
            s_mask = 0;
            cur[t] = 0; // (this array is the next sweep's `next`: it must be clear by then, and only this workgroup reads the entry)
        }
        __syncthreads();
        if (!s_dirty) continue;
        const long long t0 = t % R.n[0], t1 = (t / R.n[0]) % R.n[1], t2 = t / (R.n[0] * R.n[1]);
        const long long o[3] = {t0 * R.T[0], t1 * R.T[1], t2 * R.T[2]};
        int td[3];
        for (int a = 0; a < 3; ++a) td[a] = (int)min((long long)R.T[a], R.D[a] - o[a]);
        const int sy = td[0] + 2, sz = sy * (td[1] + 2), hv = sz * (td[2] + 2);
        uint16_t *sp = (uint16_t *)(s + hv);
        for (int i = threadIdx.x; i < hv; i += blockDim.x) {
            const int hx = i % sy, hy = (i / sy) % (td[1] + 2), hz = i / sz;
            const long long gx = o[0] + hx - 1, gy = o[1] + hy - 1, gz = o[2] + hz - 1;
            const bool in = gx >= 0 && gx < R.D[0] && gy >= 0 && gy < R.D[1] && gz >= 0 && gz < R.D[2];
            const size_t g = ((size_t)gz * R.D[1] + (size_t)gy) * R.D[0] + (size_t)gx;
            s[i] = in ? R.field[g] : MLM_REACH_BLOCKED;
            if (hx >= 1 && hx <= td[0] && hy >= 1 && hy <= td[1] && hz >= 1 && hz <= td[2]) // (a voxel of the tile: inside the box)
                sp[((hz - 1) * td[1] + hy - 1) * td[0] + hx - 1] = (uint16_t)mlm_route_pen(R.pen, R.cls[g]);
        }
        __syncthreads();
        // relax in place, a column of z per lane, down and up again; a pass without a store ends it (a lane may read a value another
        // lane stores in the same pass: older or newer, both are costs of real paths)
        const int cols = td[0] * td[1];
        int more;
        do {
            int ch = 0;
            for (int col = threadIdx.x; col < cols; col += blockDim.x) {
                const int ix = col % td[0], iy = col / td[0];
                int c = sz + (iy + 1) * sy + ix + 1, q = col;
                for (int iz = 0; iz < td[2]; ++iz, c += sz, q += cols) {
                    const uint32_t v = s[c];
                    const uint32_t w = mlm_route_relax<CONN>(v, sp[q], R.move_cost, R.max_cost, [&](int dx, int dy, int dz) { return s[c + dx + dy * sy + dz * sz]; });
                    if (w != v) {
                        s[c] = w;
                        ch = 1;
                    }
                }
                for (int iz = td[2] - 2; iz >= 0; --iz) {
                    c -= sz;
                    q -= cols;
                    const int d = c - sz;
                    const uint32_t v = s[d];
                    const uint32_t w = mlm_route_relax<CONN>(v, sp[q - cols], R.move_cost, R.max_cost, [&](int dx, int dy, int dz) { return s[d + dx + dy * sy + dz * sz]; });
                    if (w != v) {
                        s[d] = w;
                        ch = 1;
                    }
                }
            }
            more = __syncthreads_or(ch);
        } while (more);
        // write the lowered voxels back; the neighbouring tiles whose halo holds one
        uint32_t mask = 0;
        for (int col = threadIdx.x; col < cols; col += blockDim.x) {
            const int ix = col % td[0], iy = col / td[0];
            int c = sz + (iy + 1) * sy + ix + 1;
            size_t g = ((size_t)o[2] * R.D[1] + (size_t)(o[1] + iy)) * R.D[0] + (size_t)(o[0] + ix);
            for (int iz = 0; iz < td[2]; ++iz, c += sz, g += (size_t)R.D[0] * R.D[1]) {
                const uint32_t v = s[c];
                if (v < R.field[g]) { // (only this workgroup stores to its tile)
                    R.field[g] = v;
                    const unsigned faces = mlm_reach_faces(ix, iy, iz, td);
                    if (faces) mask |= mlm_route_dirty_mask(faces, CONN);
                }
            }
        }
        if (mask) atomicOr(&s_mask, mask);
        __syncthreads();
        if (threadIdx.x < 27 && ((s_mask >> threadIdx.x) & 1u)) {
            const long long nt = mlm_route_tile_at(t0, t1, t2, R.n, (int)threadIdx.x);
            if (nt >= 0) {
                next[nt] = 1;
                atomicAdd(marked, 1u);
            }
        }
    }
}

// cost / parent of the voxels [j0, j1) of the box (outputs point at voxel j0; either may be NULL) and the summary counters:
// cnt[0] traversable, cnt[1] reached, cnt[2] largest cost + 1 (0: none)
__global__ __launch_bounds__(MLM_BLOCK) void k_route_out(const MlmRoute R, long long j0, long long j1, int32_t *__restrict__ cost,
                                                         uint8_t *__restrict__ parent, unsigned long long *__restrict__ cnt) {
    __shared__ unsigned s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned n_trav = 0, n_reached = 0, top = 0;
    const long long sy = R.D[0], sz = R.D[0] * R.D[1];
    for (long long j = j0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += (long long)gridDim.x * blockDim.x) {
        const uint32_t v = R.field[j];
        if (cost) cost[j - j0] = mlm_route_cost(v);
        n_trav += v != MLM_REACH_BLOCKED;
        if (v < MLM_REACH_FAR) {
            ++n_reached;
            top = max(top, v + 1u);
        }
        if (parent) {
            uint8_t p = 255;
            if (v < MLM_REACH_FAR) {
                const long long x = j % sy, y = (j / sy) % R.D[1], z = j / sz;
                p = mlm_route_parent(v, mlm_route_pen(R.pen, R.cls[j]), R.move_cost, R.connectivity, [&](int dx, int dy, int dz) {
                    const long long ax = x + dx, ay = y + dy, az = z + dz;
                    return ax >= 0 && ax < R.D[0] && ay >= 0 && ay < R.D[1] && az >= 0 && az < R.D[2] ? R.field[j + dx + dy * sy + dz * sz]
                                                                                                      : MLM_REACH_BLOCKED;
                });
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
