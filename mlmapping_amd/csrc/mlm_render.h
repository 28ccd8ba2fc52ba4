// mlm_render.h — the pinhole arithmetic of mlm_render_depth (include/mlmap_hip.h): the segment of a pixel and the depth a stopped
// segment reports, shared by the kernel (mlm_kernels_render.h) and the CPU test driver (tests/cpp/render_driver.cpp), so that both run
// the very same arithmetic; the walk itself is mlm_raywalk.h's.  No reference counterpart: the reference projects depth images into
// the map (project_depth, mlmap.cpp:338-349) and has no inverse; the pixel convention (integer u, v; x = (u - cx) z / fx) is its own.
//
// Every operation is one IEEE double operation in the order written: a fused multiply-add would move a segment's end point by an
// ulp and with it, now and then, a lattice coordinate.  The library and the test driver are built with -ffp-contract=off; the
// pragma below holds the device code to it whatever the flags of a build that includes this header.
//
// A pose-defined variant of mlm_query_views would start from mlm_render_segment too.
#pragma once
#include "mlm_raywalk.h"

// The segment of pixel (u, v): R = rotation sensor -> world (3 x 3, row major), o = optical centre in the world, K = fx, fy, cx, cy,
// Z = the z-depth (metres, sensor frame) at which the segment ends.
MLM_RW_HD void mlm_render_segment(const double R[9], const double o[3], const double K[4], double Z, int u, int v, double p0[3], double p1[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double xs = (((double)u - K[2]) * Z) / K[0];
    const double ys = (((double)v - K[3]) * Z) / K[1];
    const double zs = Z;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        p0[a] = o[a];
        p1[a] = ((R[3 * a] * xs + R[3 * a + 1] * ys) + R[3 * a + 2] * zs) + o[a];
    }
}

// The 16UC1 pixel of a walked segment: millimetres of z-depth at which the stopping voxel is entered, never 0 for a stop (a camera
// inside an obstacle reports 1); 0 — a sensor's "no return", what the integrate calls skip — for a segment nothing stopped or an invalid one.
// The segment ends at z = max_depth_mm / 1000 and z is linear in t, so z(t) = t * max_depth_mm millimetres.
MLM_RW_HD int mlm_render_depth_mm(int status, double t, int max_depth_mm) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (status != 1) return 0;
    const double z = t * (double)max_depth_mm;
    const long long r = (long long)floor(z + 0.5);
    return (int)(r < 1 ? 1 : (r > 65535 ? 65535 : r));
}
