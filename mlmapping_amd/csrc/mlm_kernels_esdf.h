// mlm_kernels_esdf.h — truncated Euclidean distance field of a voxel box (mlm_export_esdf; no reference counterpart: the
// reference's l2esdfs_batch_3d is disabled upstream and is not a Euclidean transform, so the field is defined here, on the
// classes mlm_export_window reads out).
//
// Voxel indices, window and layout are those of mlm_export_window (mlm_kernels_window.h).  C = max_dist (1..64).  O(v) is the
// union of the predicates the flags select on the window's occ / infl classes at v; D_out(v) = min(C^2, min |v - o|^2 over
// obstacles o of the whole map), D_in the same over non-obstacles.  The host cuts the window into tiles (mlm_esdf_plan,
// mlm_host.h) and grows each by H = C - 1 + G voxels per side (G = 1 with gradients, else 0): an obstacle C or more voxels away
// on one axis is at least C^2 away, so the grown tile holds every obstacle that can lower a clamped value.  Per tile:
//  - k_esdf_mask: the window's brick walk (one hash lookup per brick of the grown tile), one byte O(v) per grown voxel;
//  - k_esdf_x:    the first 1-D pass, along x, straight from the mask: one wave per 64 outputs of a row ballots the mask bits
//                 of 192 voxels around them, and each lane takes the nearest set bit (<= C - 1 away) on either side;
//  - k_esdf_line: the y and z passes of the truncated min-plus transform f'(i) = min(C^2, min_{|k| <= C-1} f(i+k) + k^2), on
//                 64 x-columns x (TL + 2C - 2) rows staged in LDS, one column per lane;
//  - k_esdf_out:  sqdist / dist / central-difference gradients of the tile from the field of the tile +- G.
// Each pass shrinks the domain to what the next needs: x pass x in tile +- G, y pass x, y in tile +- G, z pass the tile +- G.
// Every value is an exact integer <= C^2 + (C-1)^2 < 2^16 (each pass clamps at C^2 without changing the clamped result), so the
// fields are u16, or D_out | D_in << 16 (two u16 lanes, packed arithmetic) for a signed field.
#pragma once
#include "mlm_kernels_window.h"

#define MLM_ESDF_LINE_TL 128 // rows of outputs a k_esdf_line workgroup stages (64 for a signed field: LDS <= 48.6 KB at C = 64)

typedef unsigned short mlm_u16x2 __attribute__((ext_vector_type(2)));

struct MlmEsdf {
    long long glo[3]; // grown tile origin (voxel indices)
    int gd[3];        // grown tile dims
    long long b0[3];  // blocks covering the grown tile: first block index per axis ...
    int nb[3];        // ... and count
    int flags;        // MLM_ESDF_OCC | MLM_ESDF_INFL | MLM_ESDF_UNKNOWN
    uint8_t *mask;    // [gd2][gd1][gd0]
};

// a voxel's obstacle predicate from its classes (the union of what the flags select)
__device__ __forceinline__ bool mlm_esdf_obstacle(int flags, int occ, int infl) {
    return ((flags & 1) && occ == 0) || ((flags & 2) && infl == 0) || ((flags & 4) && occ == -1);
}

__global__ __launch_bounds__(MLM_BLOCK) void k_esdf_mask(const MlmDev P, const MlmEsdf E) {
    __shared__ int s_slot;
    const long long n_bricks = (long long)E.nb[0] * E.nb[1] * E.nb[2];
    const int n = P.n;
    for (long long b = blockIdx.x; b < n_bricks; b += gridDim.x) {
        const int bx = (int)(b % E.nb[0]), by = (int)((b / E.nb[0]) % E.nb[1]), bz = (int)(b / ((long long)E.nb[0] * E.nb[1]));
        const long long gx = E.b0[0] + bx, gy = E.b0[1] + by, gz = E.b0[2] + bz;
        __syncthreads(); // (everyone has read the previous brick's slot)
        if (threadIdx.x == 0) s_slot = mlm_block_find(P, mlm_win_key(gx), mlm_win_key(gy), mlm_win_key(gz));
        __syncthreads();
        const int slot = s_slot;
        const bool collapsed = slot >= 0 && P.explore && P.blk_collapsed[slot];
        const long long x0 = max(gx * n, E.glo[0]), x1 = min(gx * n + n, E.glo[0] + E.gd[0]);
        const long long y0 = max(gy * n, E.glo[1]), y1 = min(gy * n + n, E.glo[1] + E.gd[1]);
        const long long z0 = max(gz * n, E.glo[2]), z1 = min(gz * n + n, E.glo[2] + E.gd[2]);
        const int ex = (int)(x1 - x0), ey = (int)(y1 - y0), ez = (int)(z1 - z0);
        const int nv = ex * ey * ez;
        const size_t base = (size_t)(slot >= 0 ? slot : 0) * P.cells;
        for (int j = threadIdx.x; j < nv; j += blockDim.x) {
            const int ix = j % ex, iy = (j / ex) % ey, iz = j / (ex * ey);
            const long long x = x0 + ix, y = y0 + iy, z = z0 + iz;
            const int cx = (int)(x - gx * n), cy = (int)(y - gy * n), cz = (int)(z - gz * n);
            const size_t at = base + (collapsed ? 0 : cz * n * n + cy * n + cx);
            const bool o = mlm_esdf_obstacle(E.flags, mlm_win_occ(P, slot, at), mlm_win_infl(P, slot, collapsed, at));
            E.mask[((size_t)(z - E.glo[2]) * E.gd[1] + (size_t)(y - E.glo[1])) * E.gd[0] + (size_t)(x - E.glo[0])] = (uint8_t)o;
        }
    }
}

// squared distance (clamped at C^2) from the lane's voxel to the nearest set bit of a 192-bit row piece: `prev`, `cur`, `next`
// are 64 consecutive voxels each, the lane's voxel is bit `lane` of `cur`; C - 1 <= 63, so one 64-bit look each way suffices
__device__ __forceinline__ unsigned mlm_esdf_row_dist(unsigned long long prev, unsigned long long cur, unsigned long long next, int lane,
                                                      unsigned C) {
    const unsigned long long right = (cur >> lane) | (lane ? next << (64 - lane) : 0ull);               // bit k: voxel + k
    const unsigned long long left = (cur << (63 - lane)) | (lane < 63 ? prev >> (lane + 1) : 0ull);     // bit 63 - k: voxel - k
    const unsigned dr = right ? (unsigned)__builtin_ctzll(right) : 64u, dl = left ? (unsigned)__builtin_clzll(left) : 64u;
    const unsigned d = min(dl, dr);
    return d < C ? d * d : C * C;
}

// x pass: rows = gd2 * gd1 rows of the mask, each gd0 = ex + 2C - 2 long; out [rows][ex], output j at grown x = j + C - 1.
// One wave per 64 outputs of a row (wave-uniform loop: the ballots see every lane).
template <bool SIGNED>
__global__ __launch_bounds__(MLM_BLOCK) void k_esdf_x(const uint8_t *__restrict__ mask, void *__restrict__ out_v, long long rows, int gd0,
                                                      int ex, int C) {
    const int lane = threadIdx.x & 63;
    const long long chunks = (ex + 63) / 64, tasks = rows * chunks;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long t = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < tasks; t += waves) {
        const long long r = t / chunks;
        const int j0 = (int)(t - r * chunks) * 64;
        const uint8_t *row = mask + (size_t)r * gd0;
        unsigned long long ob[3], fr[3];
        for (int w = 0; w < 3; ++w) {
            const int g = j0 + 64 * (w - 1) + lane + (C - 1);
            const bool in = g >= 0 && g < gd0;
            const bool o = in && row[in ? g : 0];
            ob[w] = __ballot(o);
            if (SIGNED) fr[w] = __ballot(in && !o);
        }
        const int j = j0 + lane;
        if (j < ex) {
            const unsigned dout = mlm_esdf_row_dist(ob[0], ob[1], ob[2], lane, (unsigned)C);
            if (SIGNED) {
                const unsigned din = mlm_esdf_row_dist(fr[0], fr[1], fr[2], lane, (unsigned)C);
                ((uint32_t *)out_v)[(size_t)r * ex + j] = dout | din << 16;
            } else {
                ((uint16_t *)out_v)[(size_t)r * ex + j] = (uint16_t)dout;
            }
        }
    }
}

__device__ __forceinline__ uint16_t mlm_esdf_step(uint16_t m, uint16_t a, uint16_t b, unsigned k2) {
    return (uint16_t)min((unsigned)m, min((unsigned)a, (unsigned)b) + k2);
}
__device__ __forceinline__ mlm_u16x2 mlm_esdf_step(mlm_u16x2 m, mlm_u16x2 a, mlm_u16x2 b, unsigned k2) {
    return __builtin_elementwise_min(m, __builtin_elementwise_min(a, b) + (mlm_u16x2)(uint16_t)k2);
}

// y / z pass: in [outer][Lout + 2C - 2][X], out [outer][Lout][X]; out(j) = min over |k| <= C - 1 of in(j + C - 1 + k) + k^2.
// A workgroup stages 64 columns x (tl + 2C - 2) rows of one outer slice in LDS; lane = column, the 4 waves take every 4th row.
template <class T>
__global__ __launch_bounds__(MLM_BLOCK) void k_esdf_line(const T *__restrict__ in, T *__restrict__ out, long long X, int Lout, int outer, int C,
                                                         int TL) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    T *s = (T *)s_dyn;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Lin = Lout + 2 * C - 2;
    const long long xc = (X + 63) / 64, lc = (Lout + TL - 1) / TL, tiles = (long long)outer * lc * xc;
    for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {
        const long long o = b / (lc * xc), rem = b - o * lc * xc;
        const int j0 = (int)(rem / xc) * TL;
        const long long x0 = (rem % xc) * 64;
        const int tl = min(TL, Lout - j0), rows = tl + 2 * C - 2;
        const bool col_in = x0 + lane < X;
        const T *src = in + ((size_t)o * Lin + j0) * (size_t)X + (size_t)x0 + lane;
        __syncthreads(); // (everyone is done with the previous tile's rows)
        for (int r = wave; r < rows; r += blockDim.x >> 6)
            if (col_in) s[r * 64 + lane] = src[(size_t)r * X];
        __syncthreads();
        if (col_in) {
            T *dst = out + ((size_t)o * Lout + j0) * (size_t)X + (size_t)x0 + lane;
            for (int j = wave; j < tl; j += blockDim.x >> 6) {
                const T *c = s + (j + C - 1) * 64 + lane;
                T m = c[0];
                unsigned k2 = 1;
                for (int k = 1; k < C; ++k) {
                    m = mlm_esdf_step(m, c[-k * 64], c[k * 64], k2);
                    k2 += 2 * k + 1;
                }
                dst[(size_t)j * X] = m;
            }
        }
    }
}

struct MlmEsdfOut {
    long long wd0, wd1;  // window dims x, y (output layout)
    long long t0[3];     // tile origin relative to the window
    int td[3];           // tile dims
    int fd[3];           // field dims = tile + 2G
    int G;               // 1: gradients
    long long out_base;  // window-flattened index that out[0] holds
    float d, inv;        // subbox_d_xyz as float; (float)(0.5 / subbox_d_xyz)
    int32_t *sqdist;
    float *dist, *grad;
};

template <bool SIGNED> __device__ __forceinline__ int mlm_esdf_sq(const void *f, size_t i) {
    if (!SIGNED) return ((const uint16_t *)f)[i];
    const uint32_t w = ((const uint32_t *)f)[i];
    return (w & 0xFFFFu) ? (int)(w & 0xFFFFu) : -(int)(w >> 16); // D_out > 0 exactly off obstacles; on them -D_in
}
__device__ __forceinline__ float mlm_esdf_dist(int sq, float d) {
    return sq >= 0 ? d * sqrtf((float)sq) : -(d * sqrtf((float)-sq)); // (sqrtf: correctly rounded under the build's flags)
}

template <bool SIGNED>
__global__ __launch_bounds__(MLM_BLOCK) void k_esdf_out(const void *__restrict__ field, const MlmEsdfOut Q) {
    const long long nt = (long long)Q.td[0] * Q.td[1] * Q.td[2];
    const size_t sy = (size_t)Q.fd[0], sz = (size_t)Q.fd[0] * Q.fd[1];
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(j % Q.td[0]), iy = (int)((j / Q.td[0]) % Q.td[1]), iz = (int)(j / ((long long)Q.td[0] * Q.td[1]));
        const size_t f = (size_t)(iz + Q.G) * sz + (size_t)(iy + Q.G) * sy + (size_t)(ix + Q.G);
        const long long o = ((Q.t0[2] + iz) * Q.wd1 + (Q.t0[1] + iy)) * Q.wd0 + (Q.t0[0] + ix) - Q.out_base;
        const int sq = mlm_esdf_sq<SIGNED>(field, f);
        if (Q.sqdist) Q.sqdist[o] = sq;
        if (Q.dist) Q.dist[o] = mlm_esdf_dist(sq, Q.d);
        if (Q.grad) {
            const size_t st[3] = {1, sy, sz};
            for (int a = 0; a < 3; ++a) {
                const float hi = mlm_esdf_dist(mlm_esdf_sq<SIGNED>(field, f + st[a]), Q.d);
                const float lo = mlm_esdf_dist(mlm_esdf_sq<SIGNED>(field, f - st[a]), Q.d);
                Q.grad[3 * o + a] = (hi - lo) * Q.inv;
            }
        }
    }
}
