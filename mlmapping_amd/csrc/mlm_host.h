// mlm_host.h — the pure host arithmetic of libmlmap_hip.so: no HIP, no device memory, no handle.
//
// Everything here must reproduce the reference's FP64/float operation order bit for bit (the results feed the device
// kernels as constants): the Eigen::Quaterniond / Sophus SO3+SE3 pieces of the frame setup (so3.cpp:36-96,127-197,
// se3.cpp:29-95), the depth-noise odds table (map_awareness.cpp:36-46,119-132, map_awareness.h:120-146), the pose
// latency compensation of the depth callback (mlmap.cpp:485-498) and the replay of libstdc++'s rehash policy.
// Kept separate so that tests/test_host_math.py can build it with g++ -fsanitize=address,undefined on the CPU and check
// it against the oracle and against the property tests the reference holds for Sophus (test_so3.cpp, test_se3.cpp).
// Build with -ffp-contract=off (the reference is an SSE2 build without FMA, CMakeLists.txt:4).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

#include "mlm_types.h"

#ifdef __HIPCC__
#define MLM_HD __host__ __device__
#else
#define MLM_HD
#endif

// cv::Mat::convertTo(CV_16UC1, 1000) of one 32FC1 pixel (mlmap.cpp:482): float product, cvRound (x86 cvtss2si: round
// half to even; NaN and anything that does not fit an int32 give INT_MIN), saturate_cast<ushort>(int).  So NaN, +-Inf
// (the REP-117 "no return" encoding) and |s| >= 2^31 become 0 — a pixel project_depth skips (mlmap.cpp:338-341) — while
// finite depths beyond 65.535 m saturate to 65535.
MLM_HD inline int mlm_cv_f32_to_u16(float v) {
    const float s = v * 1000.0f;
    if (!(s < 2147483648.0f)) return 0; // NaN, +Inf, >= 2^31: INT_MIN -> 0
    if (!(s > 0.0f)) return 0;          // negative (incl. -Inf) and zero
    const float r = rintf(s);
    return r > 65535.0f ? 65535 : (int)r;
}

// Pixels of a host depth image that the host entry points read (and upload): `height` rows of `width` pixels, `row_stride` pixels
// apart, from the first pixel of the first row to the LAST PIXEL of the last row — the padding behind the last row is not part of
// the image (include/mlmap_hip.h), so a buffer may end with its last pixel.  0 for arguments the entry points refuse.
inline size_t mlm_image_span(int width, int height, int row_stride) {
    if (width <= 0 || height <= 0 || row_stride < width) return 0;
    return (size_t)(height - 1) * (size_t)row_stride + (size_t)width;
}
// Same for `n_frames` images `frame_stride` pixels apart: up to the last pixel of the last frame.
inline size_t mlm_batch_span(int n_frames, size_t frame_stride, int width, int height, int row_stride) {
    const size_t one = mlm_image_span(width, height, row_stride);
    return n_frames <= 0 || !one ? 0 : (size_t)(n_frames - 1) * frame_stride + one;
}

// log10f of glibc 2.35 (Ubuntu 22.04: sysdeps/ieee754/flt-32/e_log10f.c on top of the table-driven logf of
// sysdeps/ieee754/flt-32/e_logf.c + logf_data.c), restated operation by operation: the hit increment of the reference is
// `logit(odd)` = log10f(odd / (1 - odd)) evaluated by the HOST's libm (map_local.h:8, map_local.cpp:159), and the log-odds
// it accumulates decide occupancy classes at a threshold, so the device must produce the same float bits.  Every step is
// an IEEE-754 double or float operation (no libm call), so the device result equals the host's bit for bit.  Checked
// against this image's libm over ALL positive finite floats (2^31 - 2^23 inputs: zero mismatches, with and without
// FMA contraction of the polynomial — the FMA ifunc variant of glibc's logf gives the same floats);
// tests/test_host_math.py repeats a strided sweep, and mlm_create compares the host's log10f with this function on the
// configuration's odds table and a sweep of the logit range before it lets the kernels use it (MlmDev::logit_exact).
// Precondition of mlm_glibc_logf_core: 0.5 <= x < 2 (what log10f hands it).
MLM_HD inline float mlm_glibc_logf_core(float x) {
    static const double T[16][2] = {
        {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
        {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
        {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
        {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
        {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
        {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
        {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
        {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2}};
    const double Ln2 = 0x1.62e42fefa39efp-1;
    const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    const unsigned int ix = __builtin_bit_cast(unsigned int, x);
    if (ix == 0x3f800000u) return 0.0f;
    const unsigned int tmp = ix - 0x3f330000u;  // OFF
    const int i = (int)((tmp >> (23 - 4)) % 16u);
    const int k = (int)tmp >> 23;               // arithmetic shift
    const unsigned int iz = ix - (tmp & (0x1ffu << 23));
    const double invc = T[i][0], logc = T[i][1];
    const double z = (double)__builtin_bit_cast(float, iz);
    const double r = z * invc - 1;              // log(x) = log1p(z/c - 1) + log(c) + k ln2
    const double y0 = logc + (double)k * Ln2;
    const double r2 = r * r;
    double y = A1 * r + A2;
    y = A0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}
MLM_HD inline float mlm_glibc_log10f(float x) {
    const float two25 = 3.3554432000e+07f, ivln10 = 4.3429449201e-01f, log10_2hi = 3.0102920532e-01f, log10_2lo = 7.9034151668e-07f;
    int hx = __builtin_bit_cast(int, x);
    int k = 0;
    if (hx < 0x00800000) { // x < 2^-126
        if ((hx & 0x7fffffff) == 0) return -two25 / __builtin_fabsf(x); // log(+-0) = -inf
        if (hx < 0) return (x - x) / (x - x);                           // log(-#) = NaN
        k -= 25;
        x *= two25; // subnormal: scale up
        hx = __builtin_bit_cast(int, x);
    }
    if (hx >= 0x7f800000) return x + x;
    k += (hx >> 23) - 127;
    const int i = (int)(((unsigned int)k & 0x80000000u) >> 31);
    hx = (hx & 0x007fffff) | ((0x7f - i) << 23);
    const float y = (float)(k + i);
    const float xm = __builtin_bit_cast(float, hx);
    const float z = y * log10_2lo + ivln10 * mlm_glibc_logf_core(xm);
    return z + y * log10_2hi;
}

// Dynamic LDS of k_apply_tiles for a tile of edge x edge columns of nz layers, blocks of n^3 voxels (byte offsets):
// per voxel its log-odds (f32) and class (u8, 0: not fetched yet); per layer the block index and cell coordinate (u32); per
// block the tile overlaps the pool address of its cell 0 (u32).  mlm_create sizes the kernel for nz = two grid heights.
struct MlmApplyLds {
    uint32_t occ, ztab, blk, total;
};
MLM_HD inline MlmApplyLds mlm_apply_lds(uint32_t edge, uint32_t nz, uint32_t n) {
    const uint32_t nv = edge * edge * nz, cx = (edge - 1u) / n + 2u, cz = (nz - 1u) / n + 2u; // (an extent of e touches <= (e - 1) / n + 2 blocks)
    MlmApplyLds L;
    L.occ = 4u * nv;
    L.ztab = (5u * nv + 3u) & ~3u;
    L.blk = L.ztab + 4u * nz;
    L.total = (L.blk + 4u * cx * cx * cz + 15u) & ~15u;
    return L;
}

// ---- LDS layouts and limits of the sector path's kernels (mlm_kernels_sector.h): pure layout arithmetic, shared by the kernels, by the
// plan mlm_create runs with (mlm_plan.h) and by the CPU tests
#define MLM_SEC_THREADS 512 // threads of a column's workgroup (k_sector also exists with 256: MlmDev::sec_tab <= 1024)
#define MLM_SEC_CHUNKS 256  // chunk descriptors staged per pass of k_sector (a column of a VGA frame has ~50)
// one hit cell of the column while k_sector works on it (16 bytes: a 2 048-entry table is 32 KB of LDS)
struct MlmSecCell {
    uint32_t key;   // low 16 bits: z * nRho + rho (nZ * nRho < 65 536), MLM_NIL = empty; high 16 bits, set once the column's lists are
                    // built (cells that need their order): where the cell's references start, in units of MLM_SEC_REF_ALIGN references
                    // from the column's first
    uint32_t tmin;  // first-touch time (min over contributions); a cell that needs its order: once the hit list has taken the time, the cell's
                    // origin for the reference pass (mlm_sec_origin, mlm_sector_refs.h)
    uint32_t kg;    // kinds (bits 0..20) | (record, kind) references of the cell << 21: counted up while the contributions are booked,
                    // counted down while the references are written (the count hands every writer its own stretch of the cell's segment)
    uint32_t cnt;   // contributions
};
#define MLM_SEC_REF_ALIGN 4u // a cell's references start at a multiple of this many (16 bytes) from the column's first
#ifndef MLM_SEC_CNT_BITS
#define MLM_SEC_CNT_BITS 21 // MlmSecCell::cnt: contributions in the low bits (mlm_limits.max_points < 2^21 on this path: a full-HD depth image),
                            // the sum of their strengths above them (mod 2^11: a wrap only makes a cell look weaker than it is)
#endif
MLM_HD inline __attribute__((always_inline)) uint32_t mlm_sec_strength(float a) { return a >= 0.875f ? 3u : (a >= 0.75f ? 2u : (a >= 0.5f ? 1u : 0u)); }
// LDS plan of k_sector (dynamic): the host computes the same offsets
struct MlmSecLds {
    uint32_t tab, miss, odds, sigma, rays, occ, multi, chunk, ray_p0, vox, aux, total;
};
// staged chunk descriptors of the record passes; between them the column's centre list (16 bits per table entry, and behind it target lists
// of the spread pass); later the list of occupied table entries (L.occ)
MLM_HD inline uint32_t mlm_sec_chunk_bytes(uint32_t TAB) {
    uint32_t b = 2u * MLM_SEC_CHUNKS * 4u;
    if (b < TAB * 2u) b = TAB * 2u;
    return (b + 15u) & ~15u;
}
// n_miss: words of the column's miss table (bit mask: nZ * RW; frontier mode keeps insertion times: nZ * nRho)
MLM_HD inline MlmSecLds mlm_sec_lds(uint32_t TAB, uint32_t n_miss, uint32_t n_rho, uint32_t n_z, bool explore) {
    MlmSecLds L;
    uint32_t o = 0;
    L.tab = o;      o += TAB * (uint32_t)sizeof(MlmSecCell);
    L.chunk = o;    o += mlm_sec_chunk_bytes(TAB);
    L.odds = o;     o += ((2u * MLM_DIFF_RANGE + 1u) * n_rho + 3u) & ~3u; // a byte per entry of the odds table: its strength
    L.sigma = o;    o += ((n_rho + 3u) & ~3u) * 4u;
    L.miss = o;     o += ((n_miss + 3u) & ~3u) * 4u;
    L.rays = o;     o += TAB * 2u;                       // table entries that start a ray
    L.occ = L.chunk;                                     // occupied table entries (= the column's unique hits): in the chunk
                                                         // staging, idle between the first record pass and the second
    L.multi = o;    if (explore) o += TAB * 4u;          // frontier mode: per table entry, the first point whose hit centre is the cell
    L.ray_p0 = o;   if (explore) o += TAB * 4u;          // frontier mode: first point of every ray start
    o = (o + 15u) & ~15u;
    L.vox = o;      o += (n_rho + n_z) * 16u;            // world voxel per axis: x, y by rho; z by z (see k_sector)
    L.aux = o;      o += n_rho * 24u;                    // per tile run along rho: tile, first rho, hits (count, offset); per rho: miss cells
                                                         // (count -> fill cursor, offset)
    L.total = (o + 15u) & ~15u;
    return L;
}
#ifndef MLM_TILE_DESC
#define MLM_TILE_DESC 128
#endif
// ^ descriptors staged per pass (a tile of a VGA frame has ~15; 128 instead of 256: 3 KB of LDS, a fifth workgroup per CU)
#define MLM_TILE_WORDS 64    // most words of a tile's column mask: MlmDev::tile_words = ceil(nPhi / 32) (sector path: nPhi <= 2048)
#define MLM_TILE_COMBOS 2048 // most blocks a tile may overlap: limit of MlmDev::tile_combos (their pool slots are kept in LDS)
struct MlmTileLds {
    uint32_t cnt, place, desc, slot, ztab, total;
};
MLM_HD inline MlmTileLds mlm_tile_lds(uint32_t n_vox, uint32_t lv_nz, uint32_t combos) {
    MlmTileLds L;
    uint32_t o = 0;
    L.cnt = o;      o += n_vox * 4u;                 // per voxel: misses | hits << 16 (the hit half doubles as the fill cursor later)
    L.place = o;    o += n_vox * 4u;                 // per touched voxel: record index in the tile | (offset of its hits, 0xFFFF: one hit) << 16
    o = (o + 15u) & ~15u;
    L.desc = o;     o += MLM_TILE_DESC * 16u + MLM_TILE_DESC * 8u; // staged descriptors + exclusive prefixes (miss cells, hits)
    L.slot = o;     o += combos * 4u + combos;           // pool slot per overlapped block + "the frame touches it" flags (combos: multiple of 4)
    o = (o + 3u) & ~3u;
    L.ztab = o;     o += ((lv_nz + 1u) & ~1u) * 4u;  // per grid z: block index << 8 ... (gz, cz) packed
    L.total = (o + 15u) & ~15u;
    return L;
}

// Tiles of mlm_export_esdf (mlm_kernels_esdf.h) for a window of D[0] x D[1] x D[2] voxels, truncation C (voxels), central
// gradients or not.  A tile is whole planes, else rows of one plane, else a piece of one row, so that its output is one
// contiguous range of the window's [D2][D1][D0] layout and a staged tile goes back in one copy.  The grown tile (the tile plus
// H = C - 1 + grad voxels per side: every obstacle that can lower a clamped value, and the gradient's neighbours) holds at most
// box_cap voxels, the tile itself at most out_cap (the staging of host destinations).  Tile origins are the multiples of T per
// axis, n[a] = ceil(D[a] / T[a]) of them, the last one cut to the window.  T[0] == 0: box_cap < (2H + 1)^3, no tile fits.
constexpr long long kEsdfBoxVoxels = 1ll << 25;           // grown tile: mask (1 B) + two fields (<= 4 B) per voxel, 288 MB
constexpr long long kEsdfMinBoxVoxels = 129ll * 129 * 129; // the smallest box every call fits: one voxel grown by H = 64
constexpr long long kEsdfStageVoxels = 1ll << 22;         // staged tile: <= 20 bytes per voxel
struct MlmEsdfPlan {
    long long T[3], n[3];
    long long H, grown; // grown: voxels of a full grown tile (the scratch the fields need)
};
inline MlmEsdfPlan mlm_esdf_plan(const long long D[3], int C, bool grad, long long box_cap, long long out_cap) {
    MlmEsdfPlan p{};
    const long long H = C - 1 + (grad ? 1 : 0), h2 = 2 * H;
    p.H = H;
    auto fits = [&](long long tx, long long ty, long long tz) { return (tx + h2) * (ty + h2) * (tz + h2) <= box_cap && tx * ty * tz <= out_cap; };
    if (fits(D[0], D[1], 1)) {
        p.T[0] = D[0];
        p.T[1] = D[1];
        p.T[2] = std::min({D[2], box_cap / ((D[0] + h2) * (D[1] + h2)) - h2, out_cap / (D[0] * D[1])});
    } else if (fits(D[0], 1, 1)) {
        p.T[0] = D[0];
        p.T[1] = std::min({D[1], box_cap / ((D[0] + h2) * (1 + h2)) - h2, out_cap / D[0]});
        p.T[2] = 1;
    } else if (fits(1, 1, 1)) {
        p.T[0] = std::min({D[0], box_cap / ((1 + h2) * (1 + h2)) - h2, out_cap});
        p.T[1] = p.T[2] = 1;
    } else {
        return p;
    }
    for (int a = 0; a < 3; ++a) p.n[a] = (D[a] + p.T[a] - 1) / p.T[a];
    p.grown = (p.T[0] + h2) * (p.T[1] + h2) * (p.T[2] + h2);
    return p;
}

// The voxel box [lo, lo + dims) of a read-out: D and nvox are its dims and voxel count in 64 bits.  0: ok; 1: a dim < 1 or lo + dims
// beyond an int32; 2: more than 2^31 - 1 voxels.  Axis by axis, so a box that is wrong in both ways reports the earlier axis' fault.
inline int mlm_box_check(const int32_t lo[3], const int32_t dims[3], long long D[3], long long &nvox) {
    nvox = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || (long long)lo[a] + dims[a] > 0x7FFFFFFFll) return 1;
        D[a] = dims[a];
        nvox *= D[a];
        if (nvox > 0x7FFFFFFFll) return 2;
    }
    return 0;
}

// The bricks (blocks of n voxels per axis) that cover [lo, lo + d) on one axis, d >= 1: the first brick's index (the floor of
// lo / n) and their count.  64-bit: the box a read-out grows around a window at the int32 edge (a halo, a truncation distance, a
// one-voxel rim) reaches past that edge.
inline void mlm_brick_cover(int n, long long lo, long long d, long long &b0, int &nb) {
    auto floor_div = [n](long long v) { return v >= 0 ? v / n : -((-v + n - 1) / n); };
    b0 = floor_div(lo);
    nb = (int)(floor_div(lo + d - 1) - b0 + 1);
}

// the parts of a kept device buffer start on multiples of 256 bytes
inline size_t mlm_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Where the channels of a read-out (inputs and outputs, `count[c]` elements of `elem[c]` bytes each) lie in one staging buffer: a
// channel that is present and staged (its memory is not the device's) takes its bytes rounded up to a multiple of 256 at off[c],
// in channel order; the others take nothing.  Returns the buffer's bytes.
inline size_t mlm_stage_layout(int n, const bool *present, const bool *staged, const size_t *elem, const size_t *count, size_t *off) {
    size_t total = 0;
    for (int c = 0; c < n; ++c) {
        off[c] = total;
        if (present[c] && staged[c]) total += mlm_align256(count[c] * elem[c]);
    }
    return total;
}

// The tiles of T[0] x T[1] x T[2] voxels that cut a box of D[0] x D[1] x D[2], z outermost and x innermost, the last tile per axis cut
// to the box: fn(org, td, out_base) with the tile's origin and extent in the box and the index of its first voxel in the box's
// [z][y][x] order.  Stops at, and returns, fn's first non-zero answer.  A plane is a box with D[2] = T[2] = 1.
template <class F> inline int mlm_for_tiles(const long long D[3], const long long T[3], F fn) {
    for (long long z0 = 0; z0 < D[2]; z0 += T[2])
        for (long long y0 = 0; y0 < D[1]; y0 += T[1])
            for (long long x0 = 0; x0 < D[0]; x0 += T[0]) {
                const long long org[3] = {x0, y0, z0};
                int td[3];
                for (int a = 0; a < 3; ++a) td[a] = (int)std::min(T[a], D[a] - org[a]);
                if (const int rc = fn(org, td, (z0 * D[1] + y0) * D[0] + x0)) return rc;
            }
    return 0;
}

// Rows per round when n rows (n >= 1) leave through a staging buffer: as many as `cap_bytes` hold at `per_row` staged bytes each,
// one at least — or the test knob's count (knob_rows > 0) — and never more than n.  per_row == 0: nothing is staged, one round.
inline size_t mlm_stage_rows(size_t n, size_t per_row, size_t cap_bytes, long long knob_rows = 0) {
    if (!per_row) return n;
    return std::min<size_t>(n, knob_rows > 0 ? (size_t)knob_rows : std::max<size_t>(1, cap_bytes / per_row));
}

// Tiles of mlm_export_grid2d (mlm_kernels_grid.h) for a plane of D[0] x D[1] cells, truncation C (cells), distances asked for or
// not: mlm_esdf_plan's rule in two dimensions.  A tile is whole rows of the plane, else a piece of one row, so that its outputs
// are one contiguous range of the plane's [D1][D0] layout.  The grown tile (the tile plus H = C - 1 cells per side with distances,
// H = 0 without) holds at most box_cap cells, the tile itself at most out_cap (the staging of host destinations; knob
// "grid_tile": any cap from one cell up, for the tests).  Tile origins are the multiples of T per axis, n[a] = ceil(D[a] / T[a])
// of them, the last one cut to the plane.  T[0] == 0: box_cap < (2H + 1)^2 or out_cap < 1, no tile fits.
constexpr long long kGridBoxCells = 1ll << 24;       // grown tile: mask (1 B) + two u16 fields per cell, 80 MB
constexpr long long kGridMinBoxCells = 127ll * 127;  // the smallest box every call fits: one cell grown by H = 63
constexpr long long kGridStageCells = 1ll << 20;     // staged tile: <= 41 bytes per cell
struct MlmGridPlan {
    long long T[2], n[2];
    long long H, grown; // grown: cells of a full grown tile
};
inline MlmGridPlan mlm_grid_plan(const long long D[2], int C, bool dist, long long box_cap, long long out_cap) {
    MlmGridPlan p{};
    const long long H = dist ? C - 1 : 0, h2 = 2 * H;
    p.H = H;
    auto fits = [&](long long tx, long long ty) { return (tx + h2) * (ty + h2) <= box_cap && tx * ty <= out_cap; };
    if (fits(D[0], 1)) {
        p.T[0] = D[0];
        p.T[1] = std::min({D[1], box_cap / (D[0] + h2) - h2, out_cap / D[0]});
    } else if (fits(1, 1)) {
        p.T[0] = std::min({D[0], box_cap / (1 + h2) - h2, out_cap});
        p.T[1] = 1;
    } else {
        return p;
    }
    for (int a = 0; a < 2; ++a) p.n[a] = (D[a] + p.T[a] - 1) / p.T[a];
    p.grown = (p.T[0] + h2) * (p.T[1] + h2);
    return p;
}
inline bool mlm_grid_tile_ok(long long cells) { return cells >= 1 && cells <= kGridStageCells; }

// Geometry, scratch and sweep cap of mlm_export_reach (mlm_kernels_reach.h, mlm_reach.h) for a box of D[0] x D[1] x D[2] voxels cut
// into tiles of T[0] x T[1] x T[2] (knob "reach_tile": T[0] | T[1] << 8 | T[2] << 16; the last tile per axis is cut to the box).
// A workgroup of k_reach_sweep stages a tile and its one-voxel halo as u32 in LDS: at most kReachHaloVoxels of them (60 KB, two
// workgroups per CU).  The whole box is resident at once: the field (4 B per voxel), the traversable mask (1 B), two dirty bytes
// per tile (this sweep's and the next one's), a control block (one "marked something" word per sweep of a group, the summary
// counters) and the seeds; each part starts on a multiple of 256 bytes.  cap: sweeps after which the field is final whatever
// the map (mlm_reach.h: a shortest path crosses at most min(max_steps, voxels - 1) tile faces, one sweep per crossing, one for
// the seeds' tiles, one that marks nothing), rounded up to whole groups by the host loop.  ok == false: a tile edge outside
// [1, 64] or a halo box beyond kReachHaloVoxels.
constexpr long long kReachTileDefault = 32 | (8 << 8) | (8 << 16);
constexpr long long kReachHaloVoxels = 15360;
constexpr long long kReachGroupDefault = 8, kReachGroupMax = 256;
constexpr long long kReachCtrlBytes = 2048; // kReachGroupMax words, then the counters
struct MlmReachPlan {
    bool ok;
    long long T[3], n[3], tiles, voxels;
    long long field_bytes, mask_bytes, dirty_bytes, seed_bytes; // (dirty_bytes: one of the two arrays)
    long long off_mask, off_dirty, off_ctrl, off_seeds, scratch_bytes;
    long long cap;
};
inline bool mlm_reach_tile_ok(long long packed) {
    if (packed < 0 || packed >> 24) return false;
    const long long t[3] = {packed & 255, (packed >> 8) & 255, (packed >> 16) & 255};
    for (int a = 0; a < 3; ++a)
        if (t[a] < 1 || t[a] > 64) return false;
    return (t[0] + 2) * (t[1] + 2) * (t[2] + 2) <= kReachHaloVoxels;
}
inline MlmReachPlan mlm_reach_plan(const long long D[3], long long tile_packed, long long n_seeds, long long max_steps) {
    MlmReachPlan p{};
    if (!mlm_reach_tile_ok(tile_packed) || D[0] < 1 || D[1] < 1 || D[2] < 1 || n_seeds < 1 || max_steps < 1) return p;
    auto up = [](long long v) { return (v + 255) & ~255ll; };
    p.voxels = 1;
    for (int a = 0; a < 3; ++a) {
        p.T[a] = (tile_packed >> (8 * a)) & 255;
        p.n[a] = (D[a] + p.T[a] - 1) / p.T[a];
        p.voxels *= D[a];
    }
    p.tiles = p.n[0] * p.n[1] * p.n[2];
    p.field_bytes = up(4 * p.voxels);
    p.mask_bytes = up(p.voxels);
    p.dirty_bytes = up(p.tiles);
    p.seed_bytes = up(12 * n_seeds);
    p.off_mask = p.field_bytes;
    p.off_dirty = p.off_mask + p.mask_bytes;
    p.off_ctrl = p.off_dirty + 2 * p.dirty_bytes;
    p.off_seeds = p.off_ctrl + kReachCtrlBytes;
    p.scratch_bytes = p.off_seeds + p.seed_bytes;
    p.cap = std::min(max_steps, p.voxels - 1) + 2;
    p.ok = true;
    return p;
}

// Geometry, scratch and sweep cap of mlm_export_route (mlm_kernels_route.h, mlm_route.h): the box is cut as mlm_reach_plan cuts it
// (knob "route_tile", same packing, same validity rule; knob "route_group": sweeps between two looks at the "marked" words, as
// "reach_group") and the scratch is laid out as mlm_reach_plan lays it out, the mask byte being the voxel's class byte (its ring,
// 255: blocked) and the control block holding, behind the "marked" words and the counters, the 64 words of the penalty table at
// kRoutePenOffset.  A workgroup of k_route_sweep stages the tile and its full one-voxel halo as u32 in LDS and, beside it, the
// entry penalty of every voxel of the tile as u16: lds_bytes = 4 * (T0 + 2)(T1 + 2)(T2 + 2) + 2 * T0 T1 T2, 17 696 B for the
// default tile (nine workgroups per CU by LDS), below 61 440 + 30 720 B for every valid tile (the tile holds fewer voxels than
// its halo box; beyond 64 KB the host raises the kernel's dynamic LDS limit, one workgroup per CU then).  cap: voxels + 1
// sweeps (mlm_route.h: an optimal path crosses at most voxels - 1 tile boundaries, one sweep per crossing, one for the seeds'
// tiles, one that marks nothing), rounded up to whole groups by the host loop.  ok == false: what mlm_reach_plan refuses of tile,
// box and seeds.
constexpr long long kRouteTileDefault = kReachTileDefault, kRouteGroupDefault = kReachGroupDefault;
constexpr long long kRoutePenOffset = 1280, kRoutePenWords = 64; // (within kReachCtrlBytes, behind kReachGroupMax words and the counters)
// The control block of mlm_export_reach / mlm_export_route in device memory, and the handle's pinned block that stands for it on the
// host: the device's "marked" words of a group (pinned: the 32- or 64-bit words the host read back last, whichever call they belong
// to), the device's counters (not used in the pinned block) and route's penalty table (pinned: staged there on its way up).
struct MlmCtrlBlock {
    union {
        uint32_t w32[kReachGroupMax];
        unsigned long long w64[kReachGroupMax / 2];
    } words;
    unsigned long long cnt[(kRoutePenOffset - kReachGroupMax * 4) / 8];
    uint32_t pen[kRoutePenWords];
    unsigned char rest[kReachCtrlBytes - kRoutePenOffset - kRoutePenWords * 4];
};
static_assert(offsetof(MlmCtrlBlock, words) == 0 && offsetof(MlmCtrlBlock, cnt) == kReachGroupMax * 4 && offsetof(MlmCtrlBlock, pen) == kRoutePenOffset &&
                  sizeof(MlmCtrlBlock) == kReachCtrlBytes,
              "the control block of mlm_reach_plan / mlm_route_plan");
struct MlmRoutePlan {
    bool ok;
    long long T[3], n[3], tiles, voxels;
    long long field_bytes, class_bytes, dirty_bytes, seed_bytes; // (dirty_bytes: one of the two arrays)
    long long off_class, off_dirty, off_ctrl, off_seeds, scratch_bytes;
    long long lds_bytes, cap;
};
inline MlmRoutePlan mlm_route_plan(const long long D[3], long long tile_packed, long long n_seeds) {
    MlmRoutePlan p{};
    const MlmReachPlan q = mlm_reach_plan(D, tile_packed, n_seeds, 1);
    if (!q.ok) return p;
    for (int a = 0; a < 3; ++a) {
        p.T[a] = q.T[a];
        p.n[a] = q.n[a];
    }
    p.tiles = q.tiles;
    p.voxels = q.voxels;
    p.field_bytes = q.field_bytes;
    p.class_bytes = q.mask_bytes;
    p.dirty_bytes = q.dirty_bytes;
    p.seed_bytes = q.seed_bytes;
    p.off_class = q.off_mask;
    p.off_dirty = q.off_dirty;
    p.off_ctrl = q.off_ctrl;
    p.off_seeds = q.off_seeds;
    p.scratch_bytes = q.scratch_bytes;
    p.lds_bytes = 4 * (p.T[0] + 2) * (p.T[1] + 2) * (p.T[2] + 2) + 2 * p.T[0] * p.T[1] * p.T[2];
    p.cap = p.voxels + 1;
    p.ok = true;
    return p;
}

// Geometry and scratch of mlm_export_clusters (mlm_kernels_cluster.h, mlm_cluster.h) for a box of D voxels cut into tiles as
// mlm_reach_plan cuts it (knob "cluster_tile", same packing, same validity rule: a workgroup of k_cluster_local keeps a tile's
// labels as u32 in LDS, fewer than the kReachHaloVoxels k_reach_sweep stages).  The whole box is resident at once: the field (4 B
// per voxel), the component sizes that become the components' numbers (4 B per voxel, read at the roots only), the mask (1 B),
// for a frontier the occ classes of the box grown by one voxel per side (1 B each), one count of kept roots per chunk of
// kClusterChunk voxels (the numbering: chunk counts, an exclusive scan over them, ranks inside each chunk), `cap` table rows of
// 128 B and a control block (the summary counters); each part starts on a multiple of 256 bytes.  ok == false: what
// mlm_reach_plan refuses of tile and box, or cap < 0.
constexpr long long kClusterTileDefault = kReachTileDefault;
constexpr long long kClusterChunk = 2048;
constexpr long long kClusterCtrlBytes = 256;
struct MlmClusterPlan {
    bool ok;
    long long T[3], n[3], tiles, voxels, chunks;
    long long field_bytes, num_bytes, mask_bytes, grown_bytes, chunk_bytes, table_bytes;
    long long off_num, off_mask, off_grown, off_chunk, off_table, off_ctrl, scratch_bytes;
};
inline MlmClusterPlan mlm_cluster_plan(const long long D[3], long long tile_packed, bool frontier, long long cap) {
    MlmClusterPlan p{};
    if (!mlm_reach_tile_ok(tile_packed) || D[0] < 1 || D[1] < 1 || D[2] < 1 || cap < 0) return p;
    auto up = [](long long v) { return (v + 255) & ~255ll; };
    p.voxels = 1;
    for (int a = 0; a < 3; ++a) {
        p.T[a] = (tile_packed >> (8 * a)) & 255;
        p.n[a] = (D[a] + p.T[a] - 1) / p.T[a];
        p.voxels *= D[a];
    }
    p.tiles = p.n[0] * p.n[1] * p.n[2];
    p.chunks = (p.voxels + kClusterChunk - 1) / kClusterChunk;
    p.field_bytes = up(4 * p.voxels);
    p.num_bytes = up(4 * p.voxels);
    p.mask_bytes = up(p.voxels);
    p.grown_bytes = frontier ? up((D[0] + 2) * (D[1] + 2) * (D[2] + 2)) : 0;
    p.chunk_bytes = up(4 * p.chunks);
    p.table_bytes = up(128 * cap);
    p.off_num = p.field_bytes;
    p.off_mask = p.off_num + p.num_bytes;
    p.off_grown = p.off_mask + p.mask_bytes;
    p.off_chunk = p.off_grown + p.grown_bytes;
    p.off_table = p.off_chunk + p.chunk_bytes;
    p.off_ctrl = p.off_table + p.table_bytes;
    p.scratch_bytes = p.off_ctrl + kClusterCtrlBytes;
    p.ok = true;
    return p;
}

namespace mlm_host {

// Does this host's libm log10f (what the reference's logit macro calls) agree with mlm_glibc_log10f?  Checked on the values the
// caller cares about (`vals`) and on a strided sweep of the positive floats between 1e-4 and 1e4 (the logit's argument for odds in
// [0.001, 0.999] and the noisy-OR results above them).
inline bool host_log10f_matches(const float *vals, size_t n) {
    auto same = [](float v) {
        const float a = ::log10f(v), b = mlm_glibc_log10f(v);
        return __builtin_bit_cast(unsigned int, a) == __builtin_bit_cast(unsigned int, b);
    };
    for (size_t i = 0; i < n; ++i)
        if (!same(vals[i])) return false;
    const unsigned int lo = __builtin_bit_cast(unsigned int, 1e-4f), hi = __builtin_bit_cast(unsigned int, 1e4f);
    for (unsigned int u = lo; u < hi; u += 4099u)
        if (!same(__builtin_bit_cast(float, u))) return false;
    const float sp[] = {0.0f, 1.0f, __builtin_inff(), 1e-45f, 1e-39f, 3.4e38f};
    for (float v : sp)
        if (!same(v)) return false;
    return true;
}

// ---- Eigen::Quaterniond / Sophus::SE3 pieces of the frame setup (so3.cpp:36-96, se3.cpp:29-95) -----------------
struct Q4 {
    double w, x, y, z;
};
struct D3 {
    double x, y, z;
};
inline Q4 q_mul(const Q4 &a, const Q4 &b) { // Eigen generic quat_product
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
inline Q4 q_norm(const Q4 &q) { // normalize(): coeffs / sqrt(x²+y²+z²+w²)
    const double n = std::sqrt(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    return {q.w / n, q.x / n, q.y / n, q.z / n};
}
inline D3 q_rot(const Q4 &q, const D3 &v) { // _transformVector
    D3 uv{q.y * v.z - q.z * v.y, q.z * v.x - q.x * v.z, q.x * v.y - q.y * v.x};
    uv = {uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
    const D3 c{q.y * uv.z - q.z * uv.y, q.z * uv.x - q.x * uv.z, q.x * uv.y - q.y * uv.x};
    return {(v.x + q.w * uv.x) + c.x, (v.y + q.w * uv.y) + c.y, (v.z + q.w * uv.z) + c.z};
}
inline Q4 q_from_R(const double m[9]) { // Eigen Quaternion(Matrix3): Shepperd, no normalisation (so3.cpp:39-40)
    auto M = [&](int r, int c) { return m[r * 3 + c]; };
    Q4 q;
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (M(2, 1) - M(1, 2)) * t;
        q.y = (M(0, 2) - M(2, 0)) * t;
        q.z = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > M(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
        double v[3];
        v[i] = 0.5 * t;
        t = 0.5 / t;
        q.w = (M(k, j) - M(j, k)) * t;
        v[j] = (M(j, i) + M(i, j)) * t;
        v[k] = (M(k, i) + M(i, k)) * t;
        q.x = v[0];
        q.y = v[1];
        q.z = v[2];
    }
    return q;
}

// ---- odds table (map_awareness.cpp:36-46,119-132; map_awareness.h:120-146) -------------------------------------
struct OddsModel {
    double dRho, noise;
    float sigma_in_dr(size_t x) const {
        float dis = (x * dRho);
        return noise * dis * dis / dRho;
    }
    static float standard_ND(float x) { // A&S 7.1.26; fabs/exp resolve to the float overloads
        const double a1 = 0.254829592, a2 = -0.284496736, a3 = 1.421413741, a4 = -1.453152027, a5 = 1.061405429;
        const double p = 0.3275911;
        int sign = 1;
        if (x < 0) sign = -1;
        x = std::fabs(x) / std::sqrt(2.0);
        const double t = 1.0 / (1.0 + p * x);
        const double y = 1.0 - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * std::exp(-x * x);
        return 0.5 * (1.0 + sign * y);
    }
    float get_odds(int diff, size_t r) const {
        if (r == 0) r = 1;
        const float up = standard_ND(static_cast<float>(diff + 0.5) / sigma_in_dr(r));
        const float down = standard_ND(static_cast<float>(diff - 0.5) / sigma_in_dr(r));
        float res = up - down < 0.001 ? 0.001 : up - down;
        res = res >= 0.999 ? 0.999 : res;
        return res;
    }
};

// Eigen Quaternion::toRotationMatrix (row major), as rot_og.matrix() in mlmap.cpp:492
inline void q_to_R(const Q4 &q, double R[9]) {
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1 - (tyy + tzz);
    R[1] = txy - twz;
    R[2] = txz + twy;
    R[3] = txy + twz;
    R[4] = 1 - (txx + tzz);
    R[5] = tyz - twx;
    R[6] = txz - twy;
    R[7] = tyz + twx;
    R[8] = 1 - (txx + tyy);
}
// SO3::logAndTheta, so3.cpp:134-175 (this Sophus version overwrites its |w| < eps branch: there is no `else`)
inline D3 so3_log(const Q4 &q, double *theta_out = nullptr) {
    const double EPS = 1e-10; // SMALL_EPS, so3.h:35
    const double n = std::sqrt((q.x * q.x + q.y * q.y) + q.z * q.z), w = q.w;
    double f;
    if (n < EPS)
        f = 2. / w - 2. * (n * n) / (w * (w * w));
    else
        f = 2 * std::atan(n / w) / n;
    if (theta_out) *theta_out = f * n;
    return D3{f * q.x, f * q.y, f * q.z};
}
// SO3::expAndTheta, so3.cpp:177-202 (SO3(Quaterniond) normalises)
inline Q4 so3_exp(const D3 &omega) {
    const double EPS = 1e-10;
    const double theta = std::sqrt((omega.x * omega.x + omega.y * omega.y) + omega.z * omega.z);
    const double half = 0.5 * theta, re = std::cos(half);
    double im;
    if (theta < EPS) {
        const double t2 = theta * theta, t4 = t2 * t2;
        im = 0.5 - 0.0208333 * t2 + 0.000260417 * t4;
    } else {
        im = std::sin(half) / theta;
    }
    return q_norm(Q4{re, im * omega.x, im * omega.y, im * omega.z});
}
// SE3 = (unit quaternion, translation): se3.cpp:60-95
struct T7 {
    Q4 q;
    D3 t;
};
inline T7 se3_mul(const T7 &a, const T7 &b) { // se3.cpp:60-66
    const D3 r = q_rot(a.q, b.t);
    return T7{q_norm(q_mul(a.q, b.q)), D3{a.t.x + r.x, a.t.y + r.y, a.t.z + r.z}};
}
inline T7 se3_inverse(const T7 &a) { // se3.cpp:76-83
    const Q4 qi = q_norm(Q4{a.q.w, -a.q.x, -a.q.y, -a.q.z});
    return T7{qi, q_rot(qi, D3{a.t.x * -1., a.t.y * -1., a.t.z * -1.})};
}
inline D3 se3_apply(const T7 &a, const D3 &p) { // se3.cpp:91-95
    const D3 r = q_rot(a.q, p);
    return D3{r.x + a.t.x, r.y + a.t.y, r.z + a.t.z};
}

// Pose latency compensation of depth_odom_input_callback, mlmap.cpp:470-498: T_wb forwarded to the image stamp by the
// linear model (rotation in the Lie algebra).  Stamps in seconds; out = q (w,x,y,z) then t.
inline void compensate_pose(const double odom_p[3], const double odom_q[4], const double odom_v[3], const double imu_w[3],
                            double t_img, double t_odom, double t_imu, double latency, double q_out[4], double t_out[3]) {
    const double gap_odom = t_img - t_odom, gap_imu = t_img - t_imu;
    const double time_gap = gap_imu - latency;
    const Q4 q = q_norm(Q4{odom_q[0], odom_q[1], odom_q[2], odom_q[3]});
    double R[9];
    q_to_R(q, R);
    const D3 rot_dot{(R[0] * imu_w[0] + R[1] * imu_w[1]) + R[2] * imu_w[2], (R[3] * imu_w[0] + R[4] * imu_w[1]) + R[5] * imu_w[2],
                     (R[6] * imu_w[0] + R[7] * imu_w[1]) + R[8] * imu_w[2]};
    const D3 lg = so3_log(q);
    const D3 rot_cp{lg.x + time_gap * rot_dot.x, lg.y + time_gap * rot_dot.y, lg.z + time_gap * rot_dot.z};
    const Q4 q_wb = so3_exp(rot_cp);
    const double dtv = gap_odom - latency;
    q_out[0] = q_wb.w;
    q_out[1] = q_wb.x;
    q_out[2] = q_wb.y;
    q_out[3] = q_wb.z;
    for (int i = 0; i < 3; ++i) t_out[i] = odom_p[i] + dtv * odom_v[i];
}

// T_ls and t_wa of one frame (map_awareness.cpp:184-186) — SURVEY.md App. C1, evaluated in that order
inline void frame_pose(const Q4 &q_bs, const D3 &t_bs, const double q_wb_in[4], const double t_wb_in[3], double q_ls_out[4],
                       double t_ls_out[3], double t_wa_out[3]) {
    const Q4 q_wb = q_norm(Q4{q_wb_in[0], q_wb_in[1], q_wb_in[2], q_wb_in[3]}); // SO3(Quaterniond), so3.cpp:43-47
    const D3 t_wb{t_wb_in[0], t_wb_in[1], t_wb_in[2]};
    // T_wa = (I, t_wb)
    const Q4 q_wa = q_norm(Q4{1, 0, 0, 0});
    // T_ws = T_wb * T_bs
    const D3 r1 = q_rot(q_wb, t_bs);
    const D3 t_ws{t_wb.x + r1.x, t_wb.y + r1.y, t_wb.z + r1.z};
    const Q4 q_ws = q_norm(q_mul(q_wb, q_bs));
    // T_wa^-1
    const Q4 q_ai = q_norm(Q4{q_wa.w, -q_wa.x, -q_wa.y, -q_wa.z});
    const D3 t_ai = q_rot(q_ai, D3{t_wb.x * -1., t_wb.y * -1., t_wb.z * -1.});
    // T_ls = T_wa^-1 * T_ws
    const D3 r2 = q_rot(q_ai, t_ws);
    const Q4 q_ls = q_norm(q_mul(q_ai, q_ws));
    q_ls_out[0] = q_ls.w;
    q_ls_out[1] = q_ls.x;
    q_ls_out[2] = q_ls.y;
    q_ls_out[3] = q_ls.z;
    t_ls_out[0] = t_ai.x + r2.x;
    t_ls_out[1] = t_ai.y + r2.y;
    t_ls_out[2] = t_ai.z + r2.z;
    t_wa_out[0] = t_wb.x;
    t_wa_out[1] = t_wb.y;
    t_wa_out[2] = t_wb.z;
}

// exact floor(i / d) for i < 2^27 as (i * m) >> s (Granlund-Montgomery: m = ceil(2^(27+L) / d), L = ceil(log2 d))
inline void div_magic(unsigned int d, unsigned long long &m, int &s) {
    int L = 0;
    while ((1ull << L) < d) ++L;
    s = 27 + L;
    m = ((1ull << s) + d - 1) / d;
}

// exact floor(i / d) for i < 2^20 (STRIP_MAGIC_MAX_I) and 1 <= d <= 2^11 (STRIP_MAGIC_MAX_D) as the high 32 bits of (2 i) * m,
// m = ceil(2^31 / d) <= 2^31: with m d = 2^31 + e, 0 <= e < d, and i = q d + r, (i m) / 2^31 = q + (r + i e / 2^31) / d, and
// i e < 2^20 * 2^11 = 2^31 keeps the bracket below r + 1 <= d.  (k_bin_sectors: a strip's row in the image, d = strips per row — a dense
// image of the sector path is at most MLM_SEC_MAX_WIDTH = 65 528 pixels wide, 2 048 strips, and has fewer than 2^15 strips,
// MlmDev::nb_cap with mlm_limits.max_points < 2^21.)  0: d is out of range.
constexpr unsigned int STRIP_MAGIC_MAX_I = 1u << 20, STRIP_MAGIC_MAX_D = 1u << 11;
inline uint32_t strip_magic(unsigned int d) {
    if (d < 1u || d > STRIP_MAGIC_MAX_D) return 0u;
    return (uint32_t)(((1ull << 31) + d - 1) / d);
}

// Bucket of a hit in the emulated container without a 64-bit remainder (k_sector).  The hash code is a 32-bit value sign-extended to
// size_t (VectorHasher, mlm_hash_rpz), the bucket `code % n` with n the container's bucket count.  For n < 2^32:
//   code >= 0   a 32-bit remainder, as Lemire's fastmod: with m = floor((2^64 - 1) / n) + 1 (mod 2^64: 0 for n = 1) the remainder of any
//               x < 2^32 is the high 64 bits of ((m * x) mod 2^64) * n — exact for all 2^32 operands and every n < 2^32 (Lemire, Kaser,
//               Kurz, "Faster remainder by direct computation", 2019, theorem 1 with N = 32, F = 64).  div_magic does not do: it
//               covers operands below 2^27 only.
//   code <  0   code = 2^64 - x with x = -(int32) code in [1, 2^31]: with c = 2^64 mod n and t = x mod n the bucket is
//               c - t (c >= t) or c + n - t (the sum may wrap 32 bits; the result, below n, does not).
// fast == 0 (n >= 2^32; a cylinder of more than 2^31 cells): the kernel keeps the 64-bit remainder.
// tests/test_bucket_mod.py checks both forms against 128-bit arithmetic.
struct MlmBktMod {
    unsigned long long n; // the bucket count
    unsigned long long m; // fastmod multiplier
    uint32_t c;           // 2^64 mod n
    uint32_t fast;        // 1: n < 2^32, the two forms above apply
};
inline MlmBktMod bkt_mod(unsigned long long n) {
    MlmBktMod B{n, 0ull, 0u, 0u};
    if (n == 0ull || n >= (1ull << 32)) return B;
    B.m = 0xFFFFFFFFFFFFFFFFull / n + 1ull;
    B.c = (uint32_t)((0xFFFFFFFFFFFFFFFFull % n + 1ull) % n);
    B.fast = 1u;
    return B;
}
MLM_HD inline uint32_t mlm_mod_u32(uint32_t x, const MlmBktMod &B) {
    const unsigned long long low = B.m * x; // (mod 2^64)
    const uint32_t n = (uint32_t)B.n;
    const unsigned long long lo = (low & 0xFFFFFFFFull) * n, hi = (low >> 32) * n + (lo >> 32); // high 64 bits of low * n: hi >> 32
    return (uint32_t)(hi >> 32);
}
// code: the sign-extended hash (mlm_hash_rpz); B.fast must be set
MLM_HD inline uint32_t mlm_bucket_fast(unsigned long long code, const MlmBktMod &B) {
    const uint32_t h = (uint32_t)code;
    if ((int32_t)h >= 0) return mlm_mod_u32(h, B);
    const uint32_t t = mlm_mod_u32(0u - h, B);
    return B.c >= t ? B.c - t : B.c + (uint32_t)B.n - t;
}

// Replay the rehash policy of libstdc++'s _Hashtable for `U` unique insertions into a cleared container.
// Returns the epochs: (number of elements present when the epoch ends, bucket count during the epoch).
// Uses the very policy object std::unordered_map uses, so it follows whatever libstdc++ this library is linked to.
inline std::vector<std::pair<size_t, size_t>> plan_epochs_for(std::__detail::_Prime_rehash_policy &pol, size_t &n_bkt, size_t U) {
    std::vector<std::pair<size_t, size_t>> ep;
    size_t n = n_bkt;
    size_t i = 0;
    while (i < U) {
        // _M_insert_unique_node: _M_need_rehash(bucket_count, element_count, 1) before linking the node
        const auto r = pol._M_need_rehash(n, i, 1);
        if (r.first) {
            if (i > 0) ep.emplace_back(i, n);
            n = r.second;
        }
        // the policy is inert while element_count + 1 <= _M_next_resize
        const size_t next = std::max<size_t>(i + 1, pol._M_next_resize);
        i = std::min(U, next);
    }
    ep.emplace_back(U, n);
    n_bkt = n;
    return ep;
}

} // namespace mlm_host
