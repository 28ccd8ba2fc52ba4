// mlm_raywalk.h — the voxel walk of mlm_query_rays (include/mlmap_hip.h): pure integer code shared by the kernel
// (mlm_kernels_rays.h), the host mirror (MapView::ray, mlm_mapview.h) and the CPU test driver (tests/cpp/ray_driver.cpp), so that
// all three run the very same arithmetic.  No reference counterpart: the reference has no segment query; the classes a ray meets
// are those of the reference's point queries (what mlm_export_window's occ / infl channels return), the path is defined here.
//
// Lattice: a coordinate x becomes q = floor((x / d) * 1024.0) (IEEE double; d = subbox_d_xyz), 1024 lattice units per voxel; a ray is
// invalid if a q is not finite, |q| >= 2^40, or an axis spans more than 2^25 units.  Voxel of q: q >> 10 (floor), so |v| <= 2^30 and
// everything below except the products of the comparison fits 32 bits.  Per axis with D = Q1 - Q0 != 0: s = sign(D), m = lattice
// units (along the axis) from Q0 to the face through which the ray leaves the current voxel, so m / |D| is the segment parameter
// of that crossing.  Exactly N = sum |e - v| steps: among the axes that have not reached the end voxel take the smallest m / |D|
// (by cross-multiplication: both factors <= 2^25 + 2^10), ties to the lowest axis; the taken (m, |D|) is the parameter at which the
// next voxel is entered; v += s, m += 1024.  The path is 6-connected, has N + 1 voxels, ends at the end voxel, and every voxel of
// it touches the closed segment (a ray through an edge or corner also visits the voxels it grazes).
//
// The classes come from a callable `int cls(const int g[3], const int c[3], bool new_block)`: block index and cell coordinate of
// the voxel (v = g * n + c), new_block when g differs from the previous call's (the callee keeps the block's slot until then: one
// lookup per block crossed).  It returns the MLM_RAY_* bits that hold at the voxel: 1 getOccupancy == OCCUPIED,
// 2 getInflateOccupancy == OCCUPIED, 4 getOccupancy == UNKNOWN — the ray stops at the first voxel with (bits & flags) != 0.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MLM_RW_HD __host__ __device__ __forceinline__
#define MLM_RW_UNROLL _Pragma("unroll") // (the per-axis arrays live in registers: no loop over them may stay a loop)
#else
#define MLM_RW_HD inline
#define MLM_RW_UNROLL
#endif

struct MlmRayResult {
    int status;   // 1 stopped, 0 reached the end, -1 invalid ray
    int voxel[3]; // the stopping voxel, or the end voxel
    double t;     // segment parameter at which the stopping voxel is entered (0 at the start voxel); 1 without a stop
    int n_steps;  // path index of the stopping voxel; N + 1 without a stop
    int n_unknown; // UNKNOWN voxels in front of the stopping voxel / on the whole path
};

struct MlmRayState {
    int g[3], c[3]; // block index and cell coordinate of the current voxel
    int s[3];       // step per axis: -1, 0, 1
    int m[3], ad[3]; // lattice units to the exit face, |D|
    int r[3];       // voxels still to go per axis
};

// q = floor((x / d) * 1024) as an integer; false: not finite or beyond 2^40
MLM_RW_HD bool mlm_ray_lattice(double x, double d, long long &q) {
    const double f = floor((x / d) * 1024.0);
    if (!(fabs(f) < 1099511627776.0)) return false; // (NaN fails)
    q = (long long)f;
    return true;
}

// Set the walk up; false: an invalid ray.  n = subbox_n.
MLM_RW_HD bool mlm_ray_setup(const double p0[3], const double p1[3], double d, int n, MlmRayState &S) {
    bool ok = true;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        long long q0 = 0, q1 = 0;
        ok = mlm_ray_lattice(p0[a], d, q0) && ok;
        ok = mlm_ray_lattice(p1[a], d, q1) && ok;
        const long long D = q1 - q0, aD = D < 0 ? -D : D;
        if (aD > (1ll << 25)) ok = false;
        const int v = (int)(q0 >> 10), e = (int)(q1 >> 10), low = (int)(q0 & 1023);
        S.s[a] = D > 0 ? 1 : (D < 0 ? -1 : 0);
        S.ad[a] = (int)aD;
        S.m[a] = D > 0 ? 1024 - low : (D < 0 ? low : 0);
        S.r[a] = ok ? (e > v ? e - v : v - e) : 0;
        const int g = v >= 0 ? v / n : -((-v + n - 1) / n);
        S.g[a] = g;
        S.c[a] = v - g * n;
    }
    return ok;
}

// One step.  Returns whether the block index changed; m_in / d_in: the parameter at which the new voxel is entered.
MLM_RW_HD bool mlm_ray_step(MlmRayState &S, int n, int &m_in, int &d_in) {
    int best = -1, bm = 0, bd = 1;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        const bool take = S.r[a] > 0 && (best < 0 || (long long)S.m[a] * bd < (long long)bm * S.ad[a]);
        if (take) {
            best = a;
            bm = S.m[a];
            bd = S.ad[a];
        }
    }
    m_in = bm;
    d_in = bd;
    bool nb = false;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) {
        if (best != a) continue;
        S.m[a] += 1024;
        S.r[a] -= 1;
        S.c[a] += S.s[a];
        if (S.c[a] >= n) {
            S.c[a] = 0;
            S.g[a] += 1;
            nb = true;
        } else if (S.c[a] < 0) {
            S.c[a] = n - 1;
            S.g[a] -= 1;
            nb = true;
        }
    }
    return nb;
}

MLM_RW_HD void mlm_ray_invalid(MlmRayResult &o) {
    o.status = -1;
    o.voxel[0] = o.voxel[1] = o.voxel[2] = 0;
    o.t = 0.0;
    o.n_steps = 0;
    o.n_unknown = 0;
}

// The whole walk of one ray.
template <class Cls> MLM_RW_HD void mlm_ray_walk(const double p0[3], const double p1[3], double d, int n, int flags, Cls &cls, MlmRayResult &o) {
    MlmRayState S;
    if (!mlm_ray_setup(p0, p1, d, n, S)) {
        mlm_ray_invalid(o);
        return;
    }
    int k = 0, unk = 0, m_in = 0, d_in = 1;
    bool nb = true, stopped = false;
    for (;;) {
        const int bits = cls(S.g, S.c, nb);
        if (bits & flags) {
            stopped = true;
            break;
        }
        unk += (bits >> 2) & 1;
        ++k;
        if ((S.r[0] | S.r[1] | S.r[2]) == 0) break;
        nb = mlm_ray_step(S, n, m_in, d_in);
    }
    o.status = stopped ? 1 : 0;
    MLM_RW_UNROLL
    for (int a = 0; a < 3; ++a) o.voxel[a] = S.g[a] * n + S.c[a];
    o.t = stopped ? (double)m_in / (double)d_in : 1.0; // (the start voxel: 0 / 1)
    o.n_steps = k;
    o.n_unknown = unk;
}
