// mlm_kernels_window.h — dense read-out of an axis-aligned box of voxels (mlm_export_window; no reference counterpart: every value
// is what the reference's queries return at the voxel, include/mlmap.h:170-295).
//
// Voxel index per axis: v = g*n + c (g block key, c cell coordinate).  The host cuts the window into tiles whose outputs are
// contiguous ranges of the window's [dz][dy][dx] layout (whole planes, whole rows or pieces of one row) and launches per tile:
//  - k_window_fill: one workgroup per brick = the intersection of the tile, grown by a halo of H voxels when gradients are asked
//    for, with one map block.  One hash lookup per brick; lanes walk the brick x-fastest (cid = cz*n*n + cy*n + cx: a row of a
//    block plane is contiguous), write the requested channels for voxels inside the tile and the odds of the whole haloed brick
//    into a dense scratch array (each voxel's FP64 pow is evaluated once).  An absent block reads no plane.
//  - k_window_grad: getOddGrad's walk (mlm_odd_grad_walk, the one k_query runs) per tile voxel; a neighbour k <= H steps away
//    along one axis is scratch[v +- k*stride], farther ones (max_iter > H) are looked up like k_query does.
#pragma once
#include "mlm_kernels.h"

#define MLM_WIN_HALO 8 // largest halo: max_iter beyond it falls back to lookups for the steps past it

struct MlmWin {
    long long wlo[3];   // window origin (voxel indices)
    int wd[3];          // window dims
    long long tlo[3];   // tile origin
    int td[3];          // tile dims
    long long hlo[3];   // haloed tile origin (= tile without gradients)
    int hd[3];          // haloed tile dims
    long long b0[3];    // blocks covering the haloed tile: first block index per axis ...
    int nb[3];          // ... and count
    long long out_base; // window-flattened index that out[0] holds (0: caller memory written in place; tile start: staging)
    int halo, max_iter;
    float *odds;
    int8_t *occ, *infl;
    double *grad;
    float *scratch; // odds of the haloed tile, [hd2][hd1][hd0]; null without gradients
};

// a block index as the int the lookups take: far outside the key range (|g| >= 2^20 names no block of the map, mlm_block_find)
// it is clamped, so that it stays an int and stays absent
__device__ __forceinline__ int mlm_win_key(long long g) { return (int)max(-(1ll << 21), min(1ll << 21, g)); }
// block index and cell coordinate of voxel index v: v = g*n + c, 0 <= c < n
__device__ __forceinline__ void mlm_win_axis(long long v, int n, int &g, int &c) {
    const long long g64 = v >= 0 ? v / n : -((-v + n - 1) / n);
    c = (int)(v - g64 * n);
    g = mlm_win_key(g64);
}

// what the occ / infl channels say of the voxel at pool index `at` (= slot * cells + cid, cid 0 in a released block) of block `slot`
// (-1: absent): getOccupancy (mlmap.h:170-193) and getInflateOccupancy (mlmap.h:195-211, UNKNOWN in released blocks).  The one
// statement of these classes for every dense read-out (k_window_fill, k_esdf_mask).
__device__ __forceinline__ int mlm_win_occ(const MlmDev &P, int slot, size_t at) {
    if (slot < 0) return -1;
    const uint8_t c = P.occ[at];
    return c == 'o' ? 0 : (c == 'f' ? 1 : -1);
}
__device__ __forceinline__ int mlm_win_infl(const MlmDev &P, int slot, bool collapsed, size_t at) {
    return (slot >= 0 && !collapsed && P.infl[at] == 'o') ? 0 : -1;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_window_fill(const MlmDev P, const MlmWin W) {
    __shared__ int s_slot;
    const long long n_bricks = (long long)W.nb[0] * W.nb[1] * W.nb[2];
    const int n = P.n;
    for (long long b = blockIdx.x; b < n_bricks; b += gridDim.x) {
        const int bx = (int)(b % W.nb[0]), by = (int)((b / W.nb[0]) % W.nb[1]), bz = (int)(b / ((long long)W.nb[0] * W.nb[1]));
        const long long gx = W.b0[0] + bx, gy = W.b0[1] + by, gz = W.b0[2] + bz;
        __syncthreads(); // (everyone has read the previous brick's slot)
        if (threadIdx.x == 0) s_slot = mlm_block_find(P, mlm_win_key(gx), mlm_win_key(gy), mlm_win_key(gz));
        __syncthreads();
        const int slot = s_slot;
        const bool collapsed = slot >= 0 && P.explore && P.blk_collapsed[slot]; // vectors of size 1: element 0 answers, mlmap.h:183,221
        // the brick: block [g*n, g*n+n) per axis cut to the haloed tile
        const long long x0 = max(gx * n, W.hlo[0]), x1 = min(gx * n + n, W.hlo[0] + W.hd[0]);
        const long long y0 = max(gy * n, W.hlo[1]), y1 = min(gy * n + n, W.hlo[1] + W.hd[1]);
        const long long z0 = max(gz * n, W.hlo[2]), z1 = min(gz * n + n, W.hlo[2] + W.hd[2]);
        const int ex = (int)(x1 - x0), ey = (int)(y1 - y0), ez = (int)(z1 - z0);
        const int nv = ex * ey * ez;
        const size_t base = (size_t)(slot >= 0 ? slot : 0) * P.cells;
        for (int j = threadIdx.x; j < nv; j += blockDim.x) {
            const int ix = j % ex, iy = (j / ex) % ey, iz = j / (ex * ey);
            const long long x = x0 + ix, y = y0 + iy, z = z0 + iz;
            const int cx = (int)(x - gx * n), cy = (int)(y - gy * n), cz = (int)(z - gz * n);
            const int cid = collapsed ? 0 : cz * n * n + cy * n + cx;
            const bool inside = x >= W.tlo[0] && x < W.tlo[0] + W.td[0] && y >= W.tlo[1] && y < W.tlo[1] + W.td[1] &&
                                z >= W.tlo[2] && z < W.tlo[2] + W.td[2];
            float odd = 0.5f; // getOdd of an absent block, mlmap.h:230
            if (slot >= 0 && (W.scratch || (inside && W.odds))) odd = mlm_logit_inv(P.log_odds[base + cid]);
            if (W.scratch) W.scratch[((z - W.hlo[2]) * W.hd[1] + (y - W.hlo[1])) * W.hd[0] + (x - W.hlo[0])] = odd;
            if (!inside) continue;
            const long long o = ((z - W.wlo[2]) * W.wd[1] + (y - W.wlo[1])) * W.wd[0] + (x - W.wlo[0]) - W.out_base;
            if (W.odds) W.odds[o] = odd;
            if (W.occ) W.occ[o] = (int8_t)mlm_win_occ(P, slot, base + cid);
            if (W.infl) W.infl[o] = (int8_t)mlm_win_infl(P, slot, collapsed, base + cid);
        }
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_window_grad(const MlmDev P, const MlmWin W) {
    const long long nt = (long long)W.td[0] * W.td[1] * W.td[2];
    const int n = P.n;
    const long long sy = W.hd[0], sz = (long long)W.hd[0] * W.hd[1];
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (long long)gridDim.x * blockDim.x) {
        const long long x = W.tlo[0] + j % W.td[0], y = W.tlo[1] + (j / W.td[0]) % W.td[1], z = W.tlo[2] + j / ((long long)W.td[0] * W.td[1]);
        int gx, gy, gz, cx, cy, cz;
        mlm_win_axis(x, n, gx, cx);
        mlm_win_axis(y, n, gy, cy);
        mlm_win_axis(z, n, gz, cz);
        // the voxel's centre, subbox_id2xyz_glb_vec (map_local.h:208-213), in k_query's operation order
        const double px = gx * P.d_glb + cx * P.d_sub + P.d_sub_half;
        const double py = gy * P.d_glb + cy * P.d_sub + P.d_sub_half;
        const double pz = gz * P.d_glb + cz * P.d_sub + P.d_sub_half;
        const long long s = ((z - W.hlo[2]) * W.hd[1] + (y - W.hlo[1])) * W.hd[0] + (x - W.hlo[0]);
        const float *sc = W.scratch;
        const int halo = W.halo;
        double rx, ry, rz;
        mlm_odd_grad_walk(P, gx, gy, gz, cz * n * n + cy * n + cx, px, py, pz, W.max_iter, sc[s],
                          [&](int ngx, int ngy, int ngz, int ncid, int d, int step) {
                              if (step > halo) return mlm_get_odd_at(P, ngx, ngy, ngz, ncid);
                              const long long st = d < 2 ? sz : (d < 4 ? sy : 1ll);
                              return sc[(d & 1) ? s - st * step : s + st * step];
                          },
                          rx, ry, rz);
        const long long o = ((z - W.wlo[2]) * W.wd[1] + (y - W.wlo[1])) * W.wd[0] + (x - W.wlo[0]) - W.out_base;
        W.grad[3 * o] = rx;
        W.grad[3 * o + 1] = ry;
        W.grad[3 * o + 2] = rz;
    }
}
