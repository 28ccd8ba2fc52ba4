// mlm_kernels_mesh.h — exact indexed surface mesh of a voxel box (mlm_export_mesh; no reference counterpart: the reference has no
// mesh, obstacle set, faces, vertices and their numbering are defined in include/mlmap_hip.h on the classes mlm_export_window
// reads out).  The rules are those of mlm_mesh.h, which the CPU test driver runs too; here they meet the map and the lanes.
//  - k_mesh_state: the brick walk of k_cluster_occ over the box grown by one voxel per side (one hash lookup per brick), one state
//                  byte per voxel (mlm_mesh_state);
//  - k_mesh_count: a lane per voxel, the face mask from the voxel's and its six neighbours' states, stored, and the faces of each
//                  chunk of kMeshChunk voxels counted; then a lane per lattice point, the vertex bit from the eight states around
//                  it, a wave's ballot stored as the word of its 64 lattice points, and the vertices of each chunk of kMeshChunk
//                  lattice points counted.  The summary counters are summed in registers, then in LDS, and reach memory with one
//                  atomic per counter and workgroup;
//  - k_mesh_scan:  exclusive scan of the two arrays of chunk counts in place (a workgroup each), the totals F and V behind them;
//  - k_mesh_verts: per chunk of lattice points the vertices before each of its 32 words (wbase), and the rows of the vertices
//                  numbered [v0, v1): number = the word's base + the set bits below the lane's;
//  - k_mesh_faces: per chunk of voxels a prefix sum of the masks' popcounts over the workgroup; the rows of the faces numbered
//                  [f0, f1), the quad's four vertex numbers each a look at wbase and bits (mlm_mesh_vertex_number).
// Nothing is ordered by an atomic: the numbers are ranks in linear order.  The states are read from global memory, not staged in
// LDS: a voxel's seven and a lattice point's eight bytes lie in three rows that neighbouring lanes and the next iteration share,
// so they come from the vector L1 / L2 — the staged form was not built.  Coordinates of a linear index come from
// multiplications (mlm_mesh_div); the brick walk divides by a brick's extents through multipliers made once per brick.
#pragma once
#include "mlm_mesh.h"
#include "mlm_kernels_window.h"

struct MlmMeshState {
    long long glo[3], gd[3]; // grown box: origin (voxel indices), dims
    long long b0[3];         // blocks covering it: first block index per axis ...
    int nb[3];               // ... and count
    int flags;
    uint8_t *out;            // [gd2][gd1][gd0]
};

// floor(j / d) for j < 2^20, 1 <= d <= 2^11 as the high word of (2 j) * m, m = ceil(2^31 / d) (mlm_host.h: strip_magic)
__device__ __forceinline__ uint32_t mlm_mesh_small_div(uint32_t j, uint32_t m) { return __umulhi(j << 1, m); }

__global__ __launch_bounds__(MLM_BLOCK) void k_mesh_state(const MlmDev P, const MlmMeshState E) {
    __shared__ int s_slot;
    const int n = P.n, flags = E.flags;
    const unsigned nbx = (unsigned)E.nb[0], nby = (unsigned)E.nb[1];
    const long long n_bricks = (long long)nbx * nby * E.nb[2];
    const long long glo0 = E.glo[0], glo1 = E.glo[1], glo2 = E.glo[2], gd0 = E.gd[0], gd1 = E.gd[1], gd2 = E.gd[2];
    const bool small = n <= 64; // (a brick of at most 2^18 voxels, extents of at most 2^6: the multipliers are exact)
    uint8_t *const out = E.out;
    // the workgroup's bricks, gridDim.x apart, as three coordinates carried from brick to brick (divisions once per workgroup)
    const unsigned step = gridDim.x, sx = step % nbx, sy = (step / nbx) % nby;
    const long long sz = step / ((long long)nbx * nby);
    unsigned bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby;
    long long bz = blockIdx.x / ((long long)nbx * nby);
    for (long long b = blockIdx.x; b < n_bricks; b += step) {
        const long long gx = E.b0[0] + bx, gy = E.b0[1] + by, gz = E.b0[2] + bz;
        const long long x0 = max(gx * n, glo0), x1 = min(gx * n + n, glo0 + gd0);
        const long long y0 = max(gy * n, glo1), y1 = min(gy * n + n, glo1 + gd1);
        const long long z0 = max(gz * n, glo2), z1 = min(gz * n + n, glo2 + gd2);
        const int ex = (int)(x1 - x0), ey = (int)(y1 - y0), ez = (int)(z1 - z0);
        __syncthreads(); // (everyone has read the previous brick's slot)
        if (threadIdx.x == 0) s_slot = mlm_block_find(P, mlm_win_key(gx), mlm_win_key(gy), mlm_win_key(gz));
        __syncthreads();
        const int slot = s_slot;
        // ceil(2^31 / extent): two 32-bit divisions per brick, none per voxel
        const uint32_t mx = (0x80000000u + (uint32_t)ex - 1u) / (uint32_t)ex, my = (0x80000000u + (uint32_t)ey - 1u) / (uint32_t)ey;
        const bool collapsed = slot >= 0 && P.explore && P.blk_collapsed[slot];
        const int nv = ex * ey * ez;
        const size_t base = (size_t)(slot >= 0 ? slot : 0) * P.cells;
        for (int j = threadIdx.x; j < nv; j += blockDim.x) {
            int row, iz;
            if (small) {
                row = (int)mlm_mesh_small_div((uint32_t)j, mx);
                iz = (int)mlm_mesh_small_div((uint32_t)row, my);
            } else {
                row = j / ex;
                iz = row / ey;
            }
            const int ix = j - row * ex, iy = row - iz * ey;
            const long long x = x0 + ix, y = y0 + iy, z = z0 + iz;
            const int cx = (int)(x - gx * n), cy = (int)(y - gy * n), cz = (int)(z - gz * n);
            const size_t at = base + (collapsed ? 0 : cz * n * n + cy * n + cx);
            const long long rx = x - glo0, ry = y - glo1, rz = z - glo2; // (grown-box coordinates; the box is 1 .. gd - 2)
            const bool inside = rx >= 1 && rx <= gd0 - 2 && ry >= 1 && ry <= gd1 - 2 && rz >= 1 && rz <= gd2 - 2;
            out[((size_t)rz * (size_t)gd1 + (size_t)ry) * (size_t)gd0 + (size_t)rx] =
                mlm_mesh_state(mlm_win_occ(P, slot, at), mlm_win_infl(P, slot, collapsed, at), flags, inside);
        }
        // the next brick of this workgroup
        bx += sx;
        by += sy;
        bz += sz;
        if (bx >= nbx) {
            bx -= nbx;
            ++by;
        }
        if (by >= nby) {
            by -= nby;
            ++bz;
        }
    }
}

struct MlmMeshArrays {
    const uint8_t *state;
    uint8_t *fmask;
    unsigned long long *bits;
    uint32_t *wbase;
    unsigned long long *fchunk, *vchunk; // counts, then bases; [chunks]: the total
    unsigned long long *cnt;             // the summary as the call returns it: [0] F, [1] V (k_mesh_scan), [2 .. 10] (k_mesh_count)
    long long fchunks, vchunks;
};

__global__ __launch_bounds__(MLM_BLOCK) void k_mesh_count(const MlmMeshGeo G, const MlmMeshArrays A) {
    __shared__ unsigned s_chunk;
    __shared__ unsigned s_sum[9];
    const long long nvox = G.nvox, nlat = G.nlat, fchunks = A.fchunks, vchunks = A.vchunks;
    const size_t gy = (size_t)G.gy, gz = (size_t)G.gz;
    const MlmMeshDiv by_d0 = G.by_d0, by_d1 = G.by_d1, by_l0 = G.by_l0, by_l1 = G.by_l1;
    const uint8_t *__restrict__ const state = A.state;
    if (threadIdx.x < 9) s_sum[threadIdx.x] = 0;
    unsigned sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // obstacles, obstacles with a face, faces per direction, faces at the box's rim
    for (long long c = blockIdx.x; c < fchunks; c += gridDim.x) {
        __syncthreads(); // (thread 0 has read the previous chunk's count)
        if (threadIdx.x == 0) s_chunk = 0;
        __syncthreads();
        unsigned faces = 0;
        const long long end = min(nvox, (c + 1) * kMeshChunk);
        for (long long j = c * kMeshChunk + threadIdx.x; j < end; j += blockDim.x) {
            uint32_t x, y, z;
            mlm_mesh_split((uint32_t)j, by_d0, by_d1, x, y, z);
            const size_t g = (size_t)(z + 1) * gz + (size_t)(y + 1) * gy + (size_t)(x + 1);
            const unsigned m = mlm_mesh_faces(state, g, gy, gz);
            A.fmask[j] = (uint8_t)m;
            faces += (unsigned)__popc(m);
            sum[0] += state[g] & 1u;
            sum[1] += m ? 1u : 0u;
            for (int a = 0; a < 6; ++a) sum[2 + a] += (m >> a) & 1u;
            sum[8] += (unsigned)__popc(m & mlm_mesh_rim(x, y, z, G.D));
        }
        if (faces) atomicAdd(&s_chunk, faces);
        __syncthreads();
        if (threadIdx.x == 0) A.fchunk[c] = s_chunk;
    }
    // (whole waves stay in the loop: the ballot sees every lane)
    for (long long c = blockIdx.x; c < vchunks; c += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) s_chunk = 0;
        __syncthreads();
        unsigned verts = 0;
        const long long end = min(nlat, (c + 1) * kMeshChunk);
        for (long long b = c * kMeshChunk; b < end; b += blockDim.x) {
            const long long L = b + threadIdx.x;
            bool v = false;
            if (L < end) {
                uint32_t k0, k1, k2;
                mlm_mesh_split((uint32_t)L, by_l0, by_l1, k0, k1, k2);
                int nrm[3];
                v = mlm_mesh_vertex(state, (size_t)k2 * gz + (size_t)k1 * gy + (size_t)k0, gy, gz, nrm);
            }
            const unsigned long long word = __ballot(v);
            if ((threadIdx.x & 63) == 0 && L < end) {
                A.bits[L >> 6] = word;
                verts += (unsigned)__popcll(word);
            }
        }
        if (verts) atomicAdd(&s_chunk, verts);
        __syncthreads();
        if (threadIdx.x == 0) A.vchunk[c] = s_chunk;
    }
    __syncthreads();
    for (int i = 0; i < 9; ++i)
        if (sum[i]) atomicAdd(&s_sum[i], sum[i]);
    __syncthreads();
    if (threadIdx.x < 9 && s_sum[threadIdx.x]) atomicAdd(&A.cnt[2 + threadIdx.x], (unsigned long long)s_sum[threadIdx.x]);
}

// exclusive scan of the chunk counts in place, the total behind them and into cnt: workgroup 0 the faces, workgroup 1 the vertices
__global__ __launch_bounds__(MLM_BLOCK) void k_mesh_scan(const MlmMeshArrays A) {
    __shared__ unsigned long long s_scan[MLM_BLOCK];
    unsigned long long *const arr = blockIdx.x == 0 ? A.fchunk : A.vchunk;
    const long long chunks = blockIdx.x == 0 ? A.fchunks : A.vchunks;
    unsigned long long carry = 0;
    for (long long b = 0; b < chunks; b += MLM_BLOCK) {
        const long long c = b + threadIdx.x;
        const unsigned long long v = c < chunks ? arr[c] : 0ull;
        __syncthreads(); // (the previous round's sums are read)
        s_scan[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < MLM_BLOCK; d <<= 1) {
            const unsigned long long add = threadIdx.x >= (unsigned)d ? s_scan[threadIdx.x - d] : 0ull;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < chunks) arr[c] = carry + s_scan[threadIdx.x] - v;
        carry += s_scan[MLM_BLOCK - 1];
    }
    if (threadIdx.x == 0) {
        arr[chunks] = carry;
        A.cnt[blockIdx.x] = carry;
    }
}

// wbase of every word, and the rows of the vertices numbered [v0, v1) (vert3 / xyz / n3 point at row v0; each may be null)
__global__ __launch_bounds__(MLM_BLOCK) void k_mesh_verts(const MlmMeshGeo G, const MlmMeshArrays A, long long v0, long long v1,
                                                          int32_t *__restrict__ vert3, float *__restrict__ xyz, int8_t *__restrict__ n3) {
    __shared__ uint32_t s_pre[64];
    const long long words = G.words, nlat = G.nlat, vchunks = A.vchunks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool rows = (vert3 || xyz || n3) && v1 > v0;
    for (long long c = blockIdx.x; c < vchunks; c += gridDim.x) {
        const unsigned long long base = A.vchunk[c], next = A.vchunk[c + 1];
        __syncthreads(); // (the previous chunk's prefixes are read)
        if (wave == 0) { // the vertices before each of the chunk's 32 words: a prefix sum over the first wave
            const long long w = c * (kMeshChunk / 64) + lane;
            const uint32_t p = lane < kMeshChunk / 64 && w < words ? (uint32_t)__popcll(A.bits[w]) : 0u;
            uint32_t incl = p;
            for (int d = 1; d < 32; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            s_pre[lane] = incl - p;
            if (lane < kMeshChunk / 64 && w < words) A.wbase[w] = (uint32_t)base + incl - p; // (V <= lattice points < 2^31)
        }
        __syncthreads();
        if (!rows || next == base || next <= (unsigned long long)v0 || base >= (unsigned long long)v1) continue; // (uniform: no vertex of the range)
        for (int i = wave; i < kMeshChunk / 64; i += MLM_BLOCK / 64) {
            const long long w = c * (kMeshChunk / 64) + i;
            if (w >= words) break;
            const unsigned long long word = A.bits[w];
            if (!((word >> lane) & 1ull)) continue;
            const long long L = w * 64 + lane;
            const long long k = (long long)base + s_pre[i] + __popcll(word & ((1ull << lane) - 1ull));
            if (k < v0 || k >= v1 || L >= nlat) continue;
            const size_t r = (size_t)(k - v0) * 3;
            mlm_mesh_vertex_row(G, A.state, (uint32_t)L, vert3 ? vert3 + r : nullptr, xyz ? xyz + r : nullptr, n3 ? n3 + r : nullptr);
        }
    }
}

// the rows of the faces numbered [f0, f1) (quads / face4 point at row f0; each may be null)
__global__ __launch_bounds__(MLM_BLOCK) void k_mesh_faces(const MlmMeshGeo G, const MlmMeshArrays A, long long f0, long long f1,
                                                          int32_t *__restrict__ quads, int32_t *__restrict__ face4) {
    __shared__ unsigned s_wave[MLM_BLOCK / 64];
    const long long nvox = G.nvox, fchunks = A.fchunks;
    const MlmMeshDiv by_d0 = G.by_d0, by_d1 = G.by_d1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long c = blockIdx.x; c < fchunks; c += gridDim.x) {
        unsigned long long base = A.fchunk[c];
        const unsigned long long next = A.fchunk[c + 1];
        if (next == base || next <= (unsigned long long)f0 || base >= (unsigned long long)f1) continue; // (uniform: no face of the range)
        const long long end = min(nvox, (c + 1) * kMeshChunk);
        // (whole workgroups stay in the loop: shuffles and barriers see every lane)
        for (long long b = c * kMeshChunk; b < end; b += blockDim.x) {
            const long long j = b + threadIdx.x;
            const unsigned m = j < end ? A.fmask[j] : 0u;
            if (!__syncthreads_or((int)m)) continue; // (most rounds hold no face: one barrier, and the previous round's totals are read)
            const unsigned p = (unsigned)__popc(m);
            unsigned incl = p;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            unsigned before = 0, total = 0;
            for (int w = 0; w < MLM_BLOCK / 64; ++w) {
                if (w < wave) before += s_wave[w];
                total += s_wave[w];
            }
            if (m) {
                long long f = (long long)base + before + (incl - p);
                uint32_t x, y, z;
                mlm_mesh_split((uint32_t)j, by_d0, by_d1, x, y, z);
                for (int a = 0; a < 6; ++a) {
                    if (!((m >> a) & 1u)) continue;
                    if (f >= f0 && f < f1) {
                        const size_t r = (size_t)(f - f0) * 4;
                        mlm_mesh_face_row(G, x, y, z, a, A.bits, A.wbase, quads ? quads + r : nullptr, face4 ? face4 + r : nullptr);
                    }
                    ++f;
                }
            }
            base += total;
        }
    }
}
