// mlm_kernels_grid.h — the map projected onto the ground plane (mlm_export_grid2d; what takes the place of the reference's
// Local2OccupancyGrid2D, include/independent_modules/l2grid2d.{h,cpp}, which is written against a dense array the reference no
// longer allocates and is disabled upstream; the classes are those of the reference's point queries, everything else is defined
// here, in integers).
//
// The cell (x, y) of the plane stands for the column of voxels (x, y, z), zlo <= z < zhi (voxel indices, window and classes as in
// mlm_export_window).  O(v) is mlm_export_esdf's predicate.  Per column: n_obs / n_unk / n_free (voxels with O, with occ == UNKNOWN,
// with occ == FREE), the lowest and the highest z with O, the nearest z with O at or below and at or above z_ref, and the UNKNOWN
// voxels strictly between those two; grid = 100 with an obstacle, else -1 with fewer than min_free FREE voxels, else 0.  The
// distance is the truncated 2-D Euclidean transform of the one-layer mask P = (grid == 100) (or grid != 0).  The host cuts the
// plane into tiles (mlm_grid_plan, mlm_host.h: whole rows, or pieces of one row, so that a tile's cell iy * td0 + ix is the
// (iy * td0 + ix)-th element behind the tile's first one in the plane's [dims1][dims0] layout) and grows each by C - 1 cells per
// side when distances are asked for.  Per tile:
//  - k_grid_columns: one workgroup per (bx, by) stack of bricks of the grown tile, one lane per column of the stack.  The slots of
//    up to MLM_GRID_STACK bricks are looked up at once (one lane each); then every lane walks its column upwards through them:
//    at one z the lanes of a wave read consecutive bytes of the brick's occ / infl plane (cid = cz*n*n + cy*n + cx, x fastest).  A
//    column's words are sums, first / last hits and a run length of ONE ascending walk, kept in registers: no LDS tables, no
//    atomics per voxel, no integer division per voxel (one per column).  An absent brick and a released one (element 0 answers)
//    are one homogeneous run, taken in closed form without reading a plane.  The workgroup adds its cells' six summary counts
//    in LDS and issues one 64-bit global atomic per word;
//  - k_esdf_x<false> / k_esdf_line<uint16_t> (mlm_kernels_esdf.h) on the mask: rows = the grown tile's rows, one outer slice;
//  - k_grid_dist_out: sqdist / dist of the tile.
#pragma once
#include "mlm_kernels_esdf.h"

#define MLM_GRID_STACK 64 // bricks of a stack whose slots are looked up together

struct MlmGrid {
    long long glo[2];         // grown tile origin x, y (voxel indices)
    int gd[2];                // grown tile dims
    long long tlo[2];         // tile origin
    int td[2];                // tile dims
    int zlo, zhi;             // the slab: zlo <= z < zhi
    long long b0[3];          // blocks covering the grown tile x the slab: first block index per axis ...
    int nb[3];                // ... and count
    int flags;                // MLM_GRID_OCC | _INFL | _UNKNOWN | _DIST_UNOBSERVED
    int min_free, z_ref;
    int8_t *grid;             // [td1][td0]; null: skipped
    int32_t *cols;            // [td1][td0][8]
    uint8_t *mask;            // [gd1][gd0]: P of the grown tile
    unsigned long long *sums; // the six summary words
};

// one column's state during its ascending walk
struct MlmGridCol {
    int n_obs, n_unk, n_free, zmin, zmax, below, above, gap;
};

// a run zr0 <= z < zr1 of voxels of one class (a single voxel: zr1 == zr0 + 1), above everything absorbed before.  `above` still at
// zhi means no obstacle at or above z_ref has been met yet — then every z so far below z_ref or in the open gap above it counts
template <bool COLS>
__device__ __forceinline__ void mlm_grid_absorb(MlmGridCol &S, int zr0, int zr1, int flags, int occ, int infl, int z_ref, int zhi) {
    const int len = zr1 - zr0;
    const bool o = mlm_esdf_obstacle(flags, occ, infl);
    S.n_obs += o ? len : 0;
    S.n_unk += occ == -1 ? len : 0;
    S.n_free += occ == 1 ? len : 0;
    if (!COLS) return;
    if (o) {
        if (S.zmin == zhi) S.zmin = zr0;
        S.zmax = zr1 - 1;
        if (zr0 <= z_ref) {
            S.below = min(z_ref, zr1 - 1);
            S.gap = 0;
        }
        if (zr1 > z_ref && S.above == zhi) S.above = max(zr0, z_ref);
    } else if (occ == -1 && S.above == zhi) {
        S.gap += len;
    }
}

template <bool COLS>
__global__ __launch_bounds__(MLM_BLOCK) void k_grid_columns(const MlmDev P, const MlmGrid G) {
    __shared__ int s_slot[MLM_GRID_STACK];
    __shared__ unsigned char s_rel[MLM_GRID_STACK];
    __shared__ unsigned long long s_sum[6];
    const int n = P.n, nn = n * n;
    const bool need_infl = (G.flags & 2) != 0;
    const long long stacks = (long long)G.nb[0] * G.nb[1];
    unsigned long long c_occ = 0, c_clear = 0, c_unobs = 0, t_obs = 0, t_unk = 0, t_free = 0; // this lane's share of the summary
    if (threadIdx.x < 6) s_sum[threadIdx.x] = 0;
    for (long long b = blockIdx.x; b < stacks; b += gridDim.x) {
        const int by = (int)(b / G.nb[0]), bx = (int)(b - (long long)by * G.nb[0]);
        const long long gx = G.b0[0] + bx, gy = G.b0[1] + by;
        const long long x0 = max(gx * n, G.glo[0]), x1 = min(gx * n + n, G.glo[0] + G.gd[0]);
        const long long y0 = max(gy * n, G.glo[1]), y1 = min(gy * n + n, G.glo[1] + G.gd[1]);
        const int ex = (int)(x1 - x0), ey = (int)(y1 - y0), nc = ex * ey;
        for (int j0 = 0; j0 < nc; j0 += blockDim.x) { // (one round unless a brick has more columns than the workgroup lanes)
            const int j = j0 + threadIdx.x;
            const bool active = j < nc;
            const int iy = active ? j / ex : 0, ix = active ? j - iy * ex : 0;
            const long long x = x0 + ix, y = y0 + iy;
            const size_t coff = (size_t)((int)(y - gy * n) * n + (int)(x - gx * n)); // the column's cell in a brick plane
            MlmGridCol S{0, 0, 0, G.zhi, G.zlo - 1, G.zlo - 1, G.zhi, 0};
            for (int c0 = 0; c0 < G.nb[2]; c0 += MLM_GRID_STACK) {
                const int cnt = min(MLM_GRID_STACK, G.nb[2] - c0);
                __syncthreads(); // (everyone is done with the previous slots)
                if ((int)threadIdx.x < cnt) {
                    const int slot = mlm_block_find(P, mlm_win_key(gx), mlm_win_key(gy), mlm_win_key(G.b0[2] + c0 + (int)threadIdx.x));
                    s_slot[threadIdx.x] = slot;
                    s_rel[threadIdx.x] = slot >= 0 && P.explore && P.blk_collapsed[slot]; // vectors of size 1: element 0 answers
                }
                __syncthreads();
                if (!active) continue;
                for (int k = 0; k < cnt; ++k) {
                    const long long gz = G.b0[2] + c0 + k;
                    const int z0 = (int)max(gz * n, (long long)G.zlo), z1 = (int)min(gz * n + n, (long long)G.zhi);
                    const int slot = s_slot[k];
                    if (slot < 0) {
                        mlm_grid_absorb<COLS>(S, z0, z1, G.flags, -1, -1, G.z_ref, G.zhi);
                    } else if (s_rel[k]) {
                        const size_t at = (size_t)slot * P.cells;
                        mlm_grid_absorb<COLS>(S, z0, z1, G.flags, mlm_win_occ(P, slot, at), -1, G.z_ref, G.zhi);
                    } else {
                        size_t at = (size_t)slot * P.cells + (size_t)(z0 - gz * n) * nn + coff;
#pragma unroll 4
                        for (int z = z0; z < z1; ++z, at += nn)
                            mlm_grid_absorb<COLS>(S, z, z + 1, G.flags, mlm_win_occ(P, slot, at), need_infl ? mlm_win_infl(P, slot, false, at) : -1,
                                                  G.z_ref, G.zhi);
                    }
                }
            }
            if (!active) continue;
            const int g = S.n_obs > 0 ? 100 : (S.n_free < G.min_free ? -1 : 0);
            if (G.mask) G.mask[(size_t)(y - G.glo[1]) * G.gd[0] + (size_t)(x - G.glo[0])] = (uint8_t)(g == 100 || ((G.flags & 16) && g != 0));
            if (x < G.tlo[0] || x >= G.tlo[0] + G.td[0] || y < G.tlo[1] || y >= G.tlo[1] + G.td[1]) continue; // (the halo: mask only)
            const size_t o = (size_t)(y - G.tlo[1]) * G.td[0] + (size_t)(x - G.tlo[0]);
            if (G.grid) G.grid[o] = (int8_t)g;
            if (COLS) {
                int32_t *w = G.cols + 8 * o;
                w[0] = S.n_obs;
                w[1] = S.n_unk;
                w[2] = S.n_free;
                w[3] = S.zmin;
                w[4] = S.zmax;
                w[5] = S.below;
                w[6] = S.above;
                w[7] = S.gap;
            }
            c_occ += g == 100;
            c_clear += g == 0;
            c_unobs += g == -1;
            t_obs += (unsigned long long)S.n_obs;
            t_unk += (unsigned long long)S.n_unk;
            t_free += (unsigned long long)S.n_free;
        }
    }
    if (!G.sums) return;
    __syncthreads();
    if (c_occ) atomicAdd(&s_sum[0], c_occ);
    if (c_clear) atomicAdd(&s_sum[1], c_clear);
    if (c_unobs) atomicAdd(&s_sum[2], c_unobs);
    if (t_obs) atomicAdd(&s_sum[3], t_obs);
    if (t_unk) atomicAdd(&s_sum[4], t_unk);
    if (t_free) atomicAdd(&s_sum[5], t_free);
    __syncthreads();
    if (threadIdx.x < 6 && s_sum[threadIdx.x]) atomicAdd(&G.sums[threadIdx.x], s_sum[threadIdx.x]);
}

// sqdist / dist of a tile from the field of its cells, [td1][td0]: cell j of the tile is element j behind the tile's first one
__global__ __launch_bounds__(MLM_BLOCK) void k_grid_dist_out(const uint16_t *__restrict__ field, long long nt, float d, int32_t *__restrict__ sqdist,
                                                             float *__restrict__ dist) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (long long)gridDim.x * blockDim.x) {
        const int sq = field[j];
        if (sqdist) sqdist[j] = sq;
        if (dist) dist[j] = mlm_esdf_dist(sq, d);
    }
}
