// mlm_mesh.h — the rules of mlm_export_mesh (include/mlmap_hip.h): pure integer code (and one FP64 expression, the vertex position)
// shared by the kernels (mlm_kernels_mesh.h) and the CPU test driver (tests/cpp/mesh_driver.cpp), so that both run the very same
// arithmetic.  No reference counterpart: the reference has no mesh; the classes behind the obstacle set are those of its point
// queries (what mlm_export_window's occ / infl channels return), faces, vertices and their numbering are defined here.
//
// The working arrays of a box of D voxels at lo:
//  - state:  one byte per voxel of the box grown by one voxel per side ([D2 + 2][D1 + 2][D0 + 2]): bit 0 "a face may start here"
//            (O(v) and v in the box), bit 1 open(v) (mlm_mesh_state);
//  - fmask:  one byte per voxel of the box: bit a = face (v, a) exists (mlm_mesh_faces);
//  - bits:   one bit per lattice point ([D2 + 1][D1 + 1][D0 + 1], 64 to a word): the point is a vertex (mlm_mesh_vertex);
//  - wbase:  one u32 per word of bits: the vertices before the word, so that the number of a vertex is a look at two words
//            (mlm_mesh_vertex_number);
//  - chunk counts of faces per kMeshChunk voxels and of vertices per kMeshChunk lattice points, scanned into chunk bases (one
//            entry more than chunks: the total).
// Every output is a function of these arrays, and they are functions of the map and the arguments: the numbering is a rank in a
// fixed order (faces by linear(v) * 6 + a, vertices by lattice index), never an order of arrival.
// Codes of directions: 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z (those of mlm_cluster.h).
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifdef __HIPCC__
#define MLM_MESH_HD __host__ __device__ __forceinline__
#else
#define MLM_MESH_HD inline
#endif

#define MLM_MESH_F_CLASSES 7 // (MLM_MESH_OCC | _INFL | _UNKNOWN of the public header)
#define MLM_MESH_F_SEEN 16   // (MLM_MESH_SEEN)
#define MLM_MESH_F_CLOSED 32 // (MLM_MESH_CLOSED)
#define MLM_MESH_ROW_I64 12  // (MLM_MESH_ROW)

// exact floor(i / d) for every i < 2^32 and 1 <= d < 2^32 without a division: the high 64 bits of i * m, m = ceil(2^64 / d) (Lemire,
// Kaser, Kurz, "Faster remainder by direct computation", 2019, theorem 1 with N = 32, F = 64 >= N + log2 d).  d == 1 has no such m
// below 2^64 and is answered directly.
struct MlmMeshDiv {
    unsigned long long m;
    uint32_t d;
};
inline MlmMeshDiv mlm_mesh_div_by(uint32_t d) { return MlmMeshDiv{d > 1u ? 0xFFFFFFFFFFFFFFFFull / d + 1ull : 0ull, d}; }
MLM_MESH_HD uint32_t mlm_mesh_div(uint32_t i, const MlmMeshDiv &v) {
    if (v.d == 1u) return i;
    const unsigned long long lo = (v.m & 0xFFFFFFFFull) * i, hi = (v.m >> 32) * i + (lo >> 32);
    return (uint32_t)(hi >> 32);
}

// Geometry of a call: what the kernels need of the box, built once on the host (mlm_mesh_geo).
struct MlmMeshGeo {
    long long D[3], lo[3];
    long long nvox, nlat, words; // voxels, lattice points, words of 64 lattice points
    long long gy, gz;            // strides of the state array: D0 + 2, (D0 + 2)(D1 + 2)
    long long ly, lz;            // strides of the lattice: D0 + 1, (D0 + 1)(D1 + 1)
    MlmMeshDiv by_d0, by_d1;     // linear voxel index -> x, y, z
    MlmMeshDiv by_l0, by_l1;     // lattice index -> kx, ky, kz
    MlmMeshDiv by_n;             // lattice coordinate -> block index and cell coordinate
    long long g0[3];             // floor(lo / n) per axis ...
    uint32_t r0[3];              // ... and lo - g0 * n
    int n, flags;
    double d_sub, d_glb;         // voxel edge, block edge (= d_sub * n as the map's geometry has it)
};
inline MlmMeshGeo mlm_mesh_geo(const long long D[3], const long long lo[3], int n, double d_sub, double d_glb, int flags) {
    MlmMeshGeo G{};
    G.nvox = G.nlat = 1;
    for (int a = 0; a < 3; ++a) {
        G.D[a] = D[a];
        G.lo[a] = lo[a];
        G.nvox *= D[a];
        G.nlat *= D[a] + 1;
        G.g0[a] = lo[a] >= 0 ? lo[a] / n : -((-lo[a] + n - 1) / n);
        G.r0[a] = (uint32_t)(lo[a] - G.g0[a] * n);
    }
    G.words = (G.nlat + 63) / 64;
    G.gy = D[0] + 2;
    G.gz = G.gy * (D[1] + 2);
    G.ly = D[0] + 1;
    G.lz = G.ly * (D[1] + 1);
    G.by_d0 = mlm_mesh_div_by((uint32_t)D[0]);
    G.by_d1 = mlm_mesh_div_by((uint32_t)D[1]);
    G.by_l0 = mlm_mesh_div_by((uint32_t)(D[0] + 1));
    G.by_l1 = mlm_mesh_div_by((uint32_t)(D[1] + 1));
    G.by_n = mlm_mesh_div_by((uint32_t)n);
    G.n = n;
    G.flags = flags;
    G.d_sub = d_sub;
    G.d_glb = d_glb;
    return G;
}

// a linear index of rows of `d0`, planes of `d1` rows (voxels of the box, or lattice points) -> its three coordinates
MLM_MESH_HD void mlm_mesh_split(uint32_t j, const MlmMeshDiv &d0, const MlmMeshDiv &d1, uint32_t &x, uint32_t &y, uint32_t &z) {
    const uint32_t row = mlm_mesh_div(j, d0);
    x = j - row * d0.d;
    z = mlm_mesh_div(row, d1);
    y = row - z * d1.d;
}

// The state byte of a voxel from its classes (occ: 0 OCCUPIED, 1 FREE, -1 UNKNOWN; infl: 0 OCCUPIED, else -1), the flags and whether
// it lies in the box.  O(v) is mlm_export_esdf's obstacle predicate (mlm_esdf_obstacle, restated here for the host); open(v) is
// "no obstacle", with SEEN also getOccupancy == FREE.  Outside the box no face starts, and with CLOSED everything there is open.
MLM_MESH_HD uint8_t mlm_mesh_state(int occ, int infl, int flags, bool inside) {
    if (!inside && (flags & MLM_MESH_F_CLOSED)) return 2;
    const bool o = ((flags & 1) && occ == 0) || ((flags & 2) && infl == 0) || ((flags & 4) && occ == -1);
    const bool open = !o && (!(flags & MLM_MESH_F_SEEN) || occ == 1);
    return (uint8_t)((o && inside ? 1 : 0) | (open ? 2 : 0));
}

// the faces of the voxel at index g of the state array: bit a = the neighbour in direction a is open
MLM_MESH_HD unsigned mlm_mesh_faces(const uint8_t *s, size_t g, size_t gy, size_t gz) {
    if (!(s[g] & 1)) return 0u;
    return ((s[g - 1] >> 1) & 1u) | (((s[g + 1] >> 1) & 1u) << 1) | (((s[g - gy] >> 1) & 1u) << 2) | (((s[g + gy] >> 1) & 1u) << 3) |
           (((s[g - gz] >> 1) & 1u) << 4) | (((s[g + gz] >> 1) & 1u) << 5);
}
// the sides of the box that box voxel (x, y, z) lies on: bit a = its neighbour in direction a is outside the box
MLM_MESH_HD unsigned mlm_mesh_rim(uint32_t x, uint32_t y, uint32_t z, const long long D[3]) {
    return (x == 0 ? 1u : 0u) | (x + 1 == D[0] ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y + 1 == D[1] ? 8u : 0u) | (z == 0 ? 16u : 0u) |
           (z + 1 == D[2] ? 32u : 0u);
}

// Lattice point k (box coordinates, 0 <= k[a] <= D[a]) is the corner shared by the eight voxels k - 1 + {0, 1}^3, which are the
// voxels k + {0, 1}^3 of the state array; g = (k2 * (D1 + 2) + k1) * (D0 + 2) + k0.  Of the twelve pairs (A, B = A + e_u) among them,
// each holds at most one face with the point as a corner: (A, +u) iff a face may start at A and B is open, else (B, -u) iff a
// face may start at B and A is open (a voxel where a face starts is an obstacle, hence not open).  Returns whether any does, and
// the sum of their outward normals.
MLM_MESH_HD bool mlm_mesh_vertex(const uint8_t *s, size_t g, size_t gy, size_t gz, int nrm[3]) {
    uint8_t c[8];
    for (int d = 0; d < 8; ++d) c[d] = s[g + (size_t)(d & 1) + (size_t)((d >> 1) & 1) * gy + (size_t)(d >> 2) * gz];
    bool any = false;
    for (int u = 0; u < 3; ++u) {
        int sum = 0;
        for (int d = 0; d < 8; ++d) {
            if (d & (1 << u)) continue;
            const uint8_t A = c[d], B = c[d | (1 << u)];
            const int plus = (A & 1) && (B & 2), minus = (B & 1) && (A & 2);
            sum += plus - minus;
            any |= plus || minus;
        }
        nrm[u] = sum;
    }
    return any;
}

// corner i (0..3) of face a of the voxel v (any coordinates; the lattice point of a voxel is its lower corner), counter-clockwise
// seen from the open side: with u = a >> 1, p = u + 1, q = u + 2 (mod 3) and b = v + (a & 1) e_u: b, b + e_p, b + e_p + e_q, b + e_q
// for odd a, and p, q swapped for even a
MLM_MESH_HD void mlm_mesh_corner(int a, int i, const long long v[3], long long k[3]) {
    const int u = a >> 1, p = u == 2 ? 0 : u + 1, q = u == 0 ? 2 : u - 1;
    const int first = (a & 1) ? p : q, second = (a & 1) ? q : p;
    for (int c = 0; c < 3; ++c) // (no indexing by u: the three stay in registers)
        k[c] = v[c] + (c == u ? (a & 1) : 0) + (c == first && (i == 1 || i == 2) ? 1 : 0) + (c == second && (i == 2 || i == 3) ? 1 : 0);
}

// the number of the vertex at lattice index L (its bit is set): the vertices before its word and those below it in the word
MLM_MESH_HD uint32_t mlm_mesh_vertex_number(const unsigned long long *bits, const uint32_t *wbase, uint32_t L) {
    const unsigned long long below = bits[L >> 6] & ((1ull << (L & 63u)) - 1ull);
#ifdef __HIP_DEVICE_COMPILE__
    return wbase[L >> 6] + (uint32_t)__popcll(below);
#else
    return wbase[L >> 6] + (uint32_t)__builtin_popcountll(below);
#endif
}

// position of lattice coordinate k = lo + kk on one axis (kk <= D, r0 < n: the sum is below 2^32): the voxel centre's formula
// (mlm_kernels_window.h) without its half voxel, in IEEE double in this order, rounded to float once
MLM_MESH_HD float mlm_mesh_pos(const MlmMeshGeo &G, int axis, uint32_t kk) {
    const uint32_t t = G.r0[axis] + kk, q = mlm_mesh_div(t, G.by_n), c = t - q * (uint32_t)G.n;
    const long long g = G.g0[axis] + (long long)q;
    const double a = (double)g * G.d_glb, b = (double)c * G.d_sub;
    return (float)(a + b);
}

// the rows of face a of box voxel (x, y, z): quad (the numbers of its four corners) and face4, each may be null
MLM_MESH_HD void mlm_mesh_face_row(const MlmMeshGeo &G, uint32_t x, uint32_t y, uint32_t z, int a, const unsigned long long *bits,
                                   const uint32_t *wbase, int32_t *quad, int32_t *face4) {
    if (quad) {
        const long long v[3] = {(long long)x, (long long)y, (long long)z};
        for (int i = 0; i < 4; ++i) {
            long long k[3];
            mlm_mesh_corner(a, i, v, k);
            quad[i] = (int32_t)mlm_mesh_vertex_number(bits, wbase, (uint32_t)(k[2] * G.lz + k[1] * G.ly + k[0]));
        }
    }
    if (face4) {
        face4[0] = (int32_t)(G.lo[0] + x);
        face4[1] = (int32_t)(G.lo[1] + y);
        face4[2] = (int32_t)(G.lo[2] + z);
        face4[3] = a;
    }
}

// the rows of the vertex at lattice index L: absolute lattice coordinates, position, normal sum; each may be null
MLM_MESH_HD void mlm_mesh_vertex_row(const MlmMeshGeo &G, const uint8_t *state, uint32_t L, int32_t *vert3, float *xyz, int8_t *n3) {
    uint32_t k[3];
    mlm_mesh_split(L, G.by_l0, G.by_l1, k[0], k[1], k[2]);
    for (int a = 0; a < 3; ++a) {
        if (vert3) vert3[a] = (int32_t)(G.lo[a] + k[a]);
        if (xyz) xyz[a] = mlm_mesh_pos(G, a, k[a]);
    }
    if (n3) {
        int nrm[3];
        mlm_mesh_vertex(state, (size_t)k[2] * (size_t)G.gz + (size_t)k[1] * (size_t)G.gy + (size_t)k[0], (size_t)G.gy, (size_t)G.gz, nrm);
        for (int a = 0; a < 3; ++a) n3[a] = (int8_t)nrm[a];
    }
}

// Scratch of mlm_export_mesh for a box of D voxels, the whole box resident at once; each part starts on a multiple of 256 bytes:
// per voxel one fmask byte and (grown box) one state byte, per lattice point one bit and a u32 per 64 of them — 3/16 byte —, per
// kMeshChunk voxels / lattice points a u64 chunk base (one more: the total), and a control block (the summary counters).
// why != 0: refused — 1: a dim below 1, 2: more than 2^31 - 1 lattice points (a vertex number would not fit an int32; the voxels,
// fewer than the lattice points, then fit too).
constexpr long long kMeshChunk = 2048;
constexpr long long kMeshCtrlBytes = 256;
constexpr long long kMeshStageRows = 1ll << 20; // rows of a range staged for host destinations (32 B per face, 27 B per vertex)
struct MlmMeshPlan {
    int why;
    long long voxels, lattice, grown, words, fchunks, vchunks;
    long long state_bytes, fmask_bytes, bits_bytes, wbase_bytes, fchunk_bytes, vchunk_bytes;
    long long off_fmask, off_bits, off_wbase, off_fchunk, off_vchunk, off_ctrl, scratch_bytes;
};
inline MlmMeshPlan mlm_mesh_plan(const long long D[3]) {
    MlmMeshPlan p{};
    p.lattice = p.voxels = p.grown = 1;
    for (int a = 0; a < 3; ++a) {
        if (D[a] < 1 || D[a] > 0x7FFFFFFFll) {
            p.why = 1;
            return p;
        }
        p.lattice *= D[a] + 1;
        if (p.lattice > 0x7FFFFFFFll) {
            p.why = 2;
            return p;
        }
        p.voxels *= D[a];
        p.grown *= D[a] + 2;
    }
    auto up = [](long long v) { return (v + 255) & ~255ll; };
    p.words = (p.lattice + 63) / 64;
    p.fchunks = (p.voxels + kMeshChunk - 1) / kMeshChunk;
    p.vchunks = (p.lattice + kMeshChunk - 1) / kMeshChunk;
    p.state_bytes = up(p.grown);
    p.fmask_bytes = up(p.voxels);
    p.bits_bytes = up(8 * p.words);
    p.wbase_bytes = up(4 * p.words);
    p.fchunk_bytes = up(8 * (p.fchunks + 1));
    p.vchunk_bytes = up(8 * (p.vchunks + 1));
    p.off_fmask = p.state_bytes;
    p.off_bits = p.off_fmask + p.fmask_bytes;
    p.off_wbase = p.off_bits + p.bits_bytes;
    p.off_fchunk = p.off_wbase + p.wbase_bytes;
    p.off_vchunk = p.off_fchunk + p.fchunk_bytes;
    p.off_ctrl = p.off_vchunk + p.vchunk_bytes;
    p.scratch_bytes = p.off_ctrl + kMeshCtrlBytes;
    return p;
}

// Argument check of mlm_export_mesh beyond the window: 0 fine, 1 flags (none of the class bits, or an unknown bit), 2 a negative
// cap, 3 a cap at odds with its arrays (a cap is 0 iff all of its arrays are null), 4 no output at all
inline int mlm_mesh_args(int flags, long long cap_faces, bool any_face_array, long long cap_verts, bool any_vert_array, bool summary) {
    if (!(flags & MLM_MESH_F_CLASSES) || (flags & ~(MLM_MESH_F_CLASSES | MLM_MESH_F_SEEN | MLM_MESH_F_CLOSED))) return 1;
    if (cap_faces < 0 || cap_verts < 0) return 2;
    if ((cap_faces == 0) == any_face_array || (cap_verts == 0) == any_vert_array) return 3;
    if (!any_face_array && !any_vert_array && !summary) return 4;
    return 0;
}
