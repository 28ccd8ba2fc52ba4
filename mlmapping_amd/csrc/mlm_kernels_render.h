// mlm_kernels_render.h — expected depth images of the map (mlm_render_depth; no reference counterpart: the reference projects depth
// images into the map and cannot ask the map for one.  The segment of a pixel is mlm_render.h's, the walk mlm_raywalk.h's over the
// classes of mlm_kernels_rays.h: per pixel exactly what mlm_query_rays answers for that segment).
//
// k_render: one wave per tile of TW x TH neighbouring pixels of one pose, one lane per pixel.  What k_rays gets from its caller, this
// kernel makes: the pose comes from 12 doubles read through the scalar cache (the tile, and so the pose, is wave-uniform), K, Z and
// the image geometry are kernel arguments, and the two end points of a ray exist in registers only — 48 bytes per ray that are never
// written or read.  The coherence k_rays can only hope for is here by construction: neighbouring pixels leave the optical centre
// through the same voxels and cross the same blocks, so the table probes and class loads of a wave fall on the same lines, and the
// lanes of a wave stop within a few steps of each other wherever the surface in front of the tile is smooth.
//
// No loop over tiles: a launch has a wave for every tile of its chunk (at most a few ten thousand workgroups).  The pose is then read
// before the kernel's first store, which lets the compiler keep it in SGPRs, and the hardware's dispatcher balances tiles whose rays
// differ in length.  The pixels of a partial tile beyond the right or the bottom edge are masked out: their lanes walk nothing, store
// nothing and count nothing.  The table's four sums are reduced over the wave first (two ballots and a butterfly), then one lane
// issues one 64-bit atomic per non-zero word: integer sums, one value whatever the order.
//
// The tile shape decides both how coherent the walks of a wave are (8 x 8: the narrowest bundle of rays) and how wide the u16 / int8
// row stores are (64 x 1: 128 and 64 contiguous bytes per wave); tools/render_rate.py times the three instantiations and DESIGN.md
// records which one is the default and why (knob "render_tile").
#pragma once
#include "mlm_kernels_rays.h"
#include "mlm_render.h"

struct MlmRender {
    const double *T;     // [n_poses][12]: R (row major) then o
    double K[4], Z;      // fx, fy, cx, cy; max_depth_mm / 1000
    int width, height, max_mm, flags;
    int tiles_x, tiles_y; // tiles per image row / column
    int q0, n_tiles;     // this launch: the first tile row (counted over all poses: pose * tiles_y + ty) and its tiles
    long long pix0;      // index of the launch's first pixel: the per-pixel outputs below start there
    uint16_t *depth;     // any output may be null
    int8_t *status;
    int32_t *voxel3, *n_unknown;
    unsigned long long *table; // [n_poses][MLM_RENDER_ROW], zeroed by the host
};

template <int TW, int TH> __global__ __launch_bounds__(MLM_BLOCK) void k_render(const MlmDev P, const MlmRender R) {
    static_assert(TW * TH == 64 && (TW & (TW - 1)) == 0, "a tile is one wave");
    const int lane = (int)(threadIdx.x & 63u);
    // (threadIdx.x >> 6 is the same in all lanes of a wave, which the compiler cannot see: readfirstlane makes everything derived from it scalar)
    const int tile = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MLM_BLOCK / 64) + (threadIdx.x >> 6)));
    if (tile >= R.n_tiles) return;
    const int q = R.q0 + tile / R.tiles_x, tx = tile - (tile / R.tiles_x) * R.tiles_x;
    const int pose = q / R.tiles_y, ty = q - pose * R.tiles_y;
    const int u = tx * TW + (lane & (TW - 1)), v = ty * TH + lane / TW;
    const bool live = u < R.width && v < R.height;
    const double *T = R.T + 12 * (size_t)pose;
    double rot[9], org[3];
    for (int k = 0; k < 9; ++k) rot[k] = T[k];
    for (int k = 0; k < 3; ++k) org[k] = T[9 + k];
    MlmRayResult o;
    mlm_ray_invalid(o);
    if (live) {
        double a[3], b[3];
        mlm_render_segment(rot, org, R.K, R.Z, u, v, a, b);
        MlmRayClasses cls{P, -1, 4, true};
        mlm_ray_walk(a, b, P.d_sub, P.n, R.flags, cls, o);
        const size_t i = (size_t)(((long long)pose * R.height + v) * R.width + u - R.pix0);
        if (R.depth) R.depth[i] = (uint16_t)mlm_render_depth_mm(o.status, o.t, R.max_mm);
        if (R.status) R.status[i] = (int8_t)o.status;
        if (R.voxel3) {
            R.voxel3[3 * i] = o.voxel[0];
            R.voxel3[3 * i + 1] = o.voxel[1];
            R.voxel3[3 * i + 2] = o.voxel[2];
        }
        if (R.n_unknown) R.n_unknown[i] = o.n_unknown;
    }
    if (!R.table) return;
    // (all 64 lanes are here: the masked ones carry an invalid result that `live` keeps out of the counts)
    const unsigned long long n_stop = __popcll(__ballot(live && o.status == 1)), n_end = __popcll(__ballot(live && o.status == 0)),
                             n_bad = __popcll(__ballot(live && o.status < 0));
    int unk = o.n_unknown; // (0 for masked and invalid lanes; at most 64 x 98 305)
    for (int w = 32; w >= 1; w >>= 1) unk += __shfl_xor(unk, w, 64);
    if (lane == 0) {
        unsigned long long *row = R.table + MLM_RENDER_ROW * (size_t)pose;
        if (n_stop) atomicAdd(row, n_stop);
        if (n_end) atomicAdd(row + 1, n_end);
        if (n_bad) atomicAdd(row + 2, n_bad);
        if (unk) atomicAdd(row + 3, (unsigned long long)unk);
    }
}
