// mlm_kernels_pack.h — the kernels of mlm_pack_blocks / mlm_unpack_blocks (include/mlmap_hip.h; the rule: mlm_pack.h).  Part of
// mlmap_hip.hip.
//
//  - k_pack_select: the live-map source.  A lane per pool slot writes mlm_delta_blocks' sort entry — the packed key of a slot the key
//    box selects, "no key" otherwise — and the host sorts (packed key, slot): the selected blocks in stream order in front.
//  - k_pack_size (pass 1): a wave per row; a block of many words loops over its 64-cell steps.  Per step a lane reads one cell of the
//    view, the six plane words are six ballots (only "is it zero" is kept), the literals and the cells on the two clamps are popcounts
//    of three more.  Per row: the record's size, its presence bits, its counts, and whether an occ / infl byte is none of 'u' 'f' 'o'.
//  - k_pack_chunks / k_pack_scan / k_pack_offsets: mlm_kernels_crop.h's three-phase prefix, over the rows' sizes in 64 bits instead of
//    over flags: sums per chunk of MLM_CROP_SLOTS_PER_CHUNK rows, one workgroup scans the chunk sums and adds the counts up (and takes
//    the minimum of the rows' error keys), every row's exclusive offset inside its chunk.  No atomic anywhere.
//  - k_pack_head, k_pack_write (pass 2): the header; a wave per row writes the directory row and the record: lane k < 6 stores plane
//    k's word of the step where pass 1 found the plane present, a literal goes to the rank "popcount of the lanes below + running base"
//    where that rank is below pass 1's count.  Every store lies inside the record pass 1 sized.
//  - k_unpack_check / k_unpack_write: the decoder in the same shape.  A wave per block opens its record behind the bound checks of
//    mlm_pack.h, its lanes take the plane words; the row's verdict and counts go through k_pack_chunks / k_pack_scan.  The writer
//    rebuilds a step's 64 cells from the six words: a literal's index is again a popcount of the lanes below plus the running base.
#pragma once
#include "mlm_kernels_delta.h"
#include "mlm_pack.h"

#define MLM_PACK_COLS 8 // uint64 per chunk and of the totals: units (scanned), rows, blank rows, literals, lo_min cells, lo_max cells, error key (min), 0

struct MlmPack {
    // the rows [r0, r1) of a dump (keys != null; the arrays start at row r0; infl may be null) ...
    const int32_t *keys;
    const float *lo;
    const uint8_t *occ, *infl;
    // ... or the live map: row r is the block at sorted position r (a position without a key is no row)
    const unsigned long long *sorted;
    const uint32_t *sorted_slot;
    unsigned int nb;                // slots in use (live)
    unsigned int n, r0, r1;         // rows in all; the rows of this launch
    uint32_t C, W, min_bits, max_bits;
    int32_t no_infl;
    MlmPackRow *row;                // [n] pass 1's answer
    const unsigned long long *off;  // [n] the records' offsets in units behind the directory (pass 2)
    unsigned long long base_units;  // header + directory, in units (pass 2)
    uint8_t *stream;                // (pass 2)
};

struct MlmPackSrc {
    const float *lo;
    const uint8_t *occ, *infl; // infl null: 'u'
    const int32_t *key;
    bool whole; // a released block: element 0 answers
};

// the planes of row r, or false: no such row
__device__ __forceinline__ bool mlm_pack_source(const MlmDev &P, const MlmPack &K, unsigned int r, MlmPackSrc &R) {
    const size_t C = K.C;
    if (K.keys) {
        const size_t o = (size_t)(r - K.r0);
        R.key = K.keys + 3 * o, R.lo = K.lo + o * C, R.occ = K.occ + o * C;
        R.infl = K.infl && !K.no_infl ? K.infl + o * C : nullptr;
        R.whole = false;
        return true;
    }
    if (K.sorted[r] == MLM_WARP_EMPTY) return false;
    const unsigned int s = K.sorted_slot[r];
    if (s >= K.nb) return false; // (never: the sort's values are the slots)
    R.whole = P.explore && P.blk_collapsed[s];
    R.key = P.block_keys + 3 * (size_t)s, R.lo = P.log_odds + (size_t)s * C, R.occ = P.occ + (size_t)s * C;
    R.infl = R.whole || K.no_infl ? nullptr : P.infl + (size_t)s * C;
    return true;
}
// cell c of a row's view as codes; false: a byte outside 'u' 'f' 'o' (its code reads 0).  c >= C reads blank.
__device__ __forceinline__ bool mlm_pack_cell(const MlmPackSrc &R, const MlmPack &K, uint32_t c, uint32_t &bits, uint32_t &co, uint32_t &ci, uint32_t &cv) {
    bits = co = ci = cv = 0u;
    if (c >= K.C) return true;
    const size_t at = R.whole ? 0 : c;
    bits = mlm_fuse_bits(R.lo[at]);
    co = mlm_pack_class_code(R.occ[at]);
    ci = R.infl ? mlm_pack_class_code(R.infl[at]) : 0u;
    cv = mlm_pack_val_code(bits, K.min_bits, K.max_bits);
    const bool ok = co != 3u && ci != 3u;
    if (co == 3u) co = 0u;
    if (ci == 3u) ci = 0u;
    return ok;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_pack_select(const MlmDev P, const MlmAgeSel S, unsigned int nb, unsigned long long *__restrict__ packed,
                                                           uint32_t *__restrict__ slot_of) {
    for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < nb; s += (unsigned long long)gridDim.x * blockDim.x) {
        const int32_t *key = P.block_keys + 3 * (size_t)s;
        const int g[3] = {key[0], key[1], key[2]};
        packed[s] = mlm_age_selects(S, g[0], g[1], g[2]) ? mlm_warp_pack(g) : MLM_WARP_EMPTY;
        slot_of[s] = (uint32_t)s;
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_pack_size(const MlmDev P, const MlmPack K) {
    const int lane = threadIdx.x & 63;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64), r1 = K.r1;
    const uint32_t W = K.W;
    MlmPackRow *const rows = K.row;
    for (unsigned int r = K.r0 + blockIdx.x * (MLM_BLOCK / 64) + wave; r < r1; r += waves) {
        MlmPackRow out{};
        MlmPackSrc R;
        if (mlm_pack_source(P, K, r, R)) { // (wave-uniform)
            uint32_t pres = 0, n_lit = 0, n_min = 0, n_max = 0;
            bool bad = false;
            for (uint32_t j = 0; j < W; ++j) {
                uint32_t bits, co, ci, cv;
                const bool ok = mlm_pack_cell(R, K, 64u * j + (uint32_t)lane, bits, co, ci, cv);
                pres |= (__ballot(co & 1u) ? 1u : 0u) | (__ballot(co & 2u) ? 2u : 0u) | (__ballot(ci & 1u) ? 4u : 0u) | (__ballot(ci & 2u) ? 8u : 0u) |
                        (__ballot(cv & 1u) ? 16u : 0u) | (__ballot(cv & 2u) ? 32u : 0u);
                n_lit += (uint32_t)__builtin_popcountll(__ballot(cv == 3u));
                n_min += (uint32_t)__builtin_popcountll(__ballot(cv == 1u));
                n_max += (uint32_t)__builtin_popcountll(__ballot(cv == 2u));
                bad = bad || __ballot(!ok) != 0ull;
            }
            out.units = (uint32_t)(mlm_pack_record_bytes(W, pres, n_lit) / 8ull);
            out.n_lit = n_lit, out.n_min = n_min, out.n_max = n_max, out.presence = pres, out.err = bad ? 1u : 0u, out.pad0 = 1u;
        }
        if (lane == 0) rows[r] = out;
    }
}

// the sums of a workgroup's lanes: columns 0 .. 5 added, column 6 the minimum; the result is in every thread k < MLM_PACK_COLS - 1
__device__ __forceinline__ unsigned long long mlm_pack_reduce(const unsigned long long (&acc)[MLM_PACK_COLS]) {
    __shared__ unsigned long long s_red[MLM_BLOCK / 64][MLM_PACK_COLS];
    const int lane = threadIdx.x & 63;
    __syncthreads(); // (the previous use is read)
#pragma unroll
    for (int k = 0; k < MLM_PACK_COLS - 1; ++k) {
        unsigned long long v = acc[k];
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(v, off);
            v = k == 6 ? (o < v ? o : v) : v + o;
        }
        if (lane == 0) s_red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    unsigned long long t = 0;
    if (threadIdx.x < MLM_PACK_COLS - 1) {
        t = s_red[0][threadIdx.x];
        for (int w = 1; w < MLM_BLOCK / 64; ++w) t = threadIdx.x == 6 ? (s_red[w][6] < t ? s_red[w][6] : t) : t + s_red[w][threadIdx.x];
    }
    return t;
}

// phase 1 of the prefix: the columns of every chunk of rows.  next_err (null: none): what row i - 1 found wrong with row i.
__global__ __launch_bounds__(MLM_BLOCK) void k_pack_chunks(const MlmPackRow *__restrict__ row, const uint32_t *__restrict__ next_err, unsigned int n, unsigned int chunks,
                                                           unsigned long long *__restrict__ chunk_sum) {
    for (unsigned int c = blockIdx.x; c < chunks; c += gridDim.x) {
        unsigned long long acc[MLM_PACK_COLS] = {};
        acc[6] = ~0ull;
        for (unsigned int k = 0; k < MLM_CROP_SLOTS_PER_CHUNK; k += MLM_BLOCK) {
            const unsigned long long i = (unsigned long long)c * MLM_CROP_SLOTS_PER_CHUNK + k + threadIdx.x;
            if (i >= n) continue;
            const MlmPackRow R = row[i];
            acc[0] += R.units, acc[1] += R.pad0, acc[2] += (R.pad0 && R.units == 1u) ? 1u : 0u, acc[3] += R.n_lit, acc[4] += R.n_min, acc[5] += R.n_max;
            const unsigned long long key = mlm_pack_verdict_key((uint32_t)i, R.err, next_err ? next_err[i] : 0u);
            if (key < acc[6]) acc[6] = key;
        }
        const unsigned long long t = mlm_pack_reduce(acc);
        if (threadIdx.x < MLM_PACK_COLS - 1) chunk_sum[(size_t)c * MLM_PACK_COLS + threadIdx.x] = t;
    }
}

// phase 2: one workgroup; column 0 of the chunks scanned in place (exclusive), the totals of all columns
__global__ __launch_bounds__(MLM_BLOCK) void k_pack_scan(unsigned long long *__restrict__ chunk_sum, unsigned int chunks, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long s_scan[MLM_BLOCK];
    unsigned long long carry = 0;
    unsigned long long acc[MLM_PACK_COLS] = {};
    acc[6] = ~0ull;
    for (unsigned int b = 0; b < chunks; b += MLM_BLOCK) {
        const unsigned int c = b + threadIdx.x;
        const unsigned long long v = c < chunks ? chunk_sum[(size_t)c * MLM_PACK_COLS] : 0ull;
        if (c < chunks) {
            for (int k = 1; k < 6; ++k) acc[k] += chunk_sum[(size_t)c * MLM_PACK_COLS + k];
            const unsigned long long key = chunk_sum[(size_t)c * MLM_PACK_COLS + 6];
            if (key < acc[6]) acc[6] = key;
        }
        __syncthreads(); // (the previous round's sums are read)
        s_scan[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < MLM_BLOCK; d <<= 1) {
            const unsigned long long add = threadIdx.x >= (unsigned int)d ? s_scan[threadIdx.x - d] : 0ull;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < chunks) chunk_sum[(size_t)c * MLM_PACK_COLS] = carry + s_scan[threadIdx.x] - v;
        carry += s_scan[MLM_BLOCK - 1];
    }
    const unsigned long long t = mlm_pack_reduce(acc);
    if (threadIdx.x == 0) totals[0] = carry;
    else if (threadIdx.x < MLM_PACK_COLS - 1) totals[threadIdx.x] = t;
    if (threadIdx.x == MLM_PACK_COLS - 1) totals[threadIdx.x] = 0ull;
}

// phase 3: off[i] = the units of the rows below i; a thread takes MLM_CROP_SLOTS_PER_CHUNK / MLM_BLOCK consecutive rows of a chunk
__global__ __launch_bounds__(MLM_BLOCK) void k_pack_offsets(const MlmPackRow *__restrict__ row, unsigned int n, unsigned int chunks,
                                                            const unsigned long long *__restrict__ chunk_sum, unsigned long long *__restrict__ off) {
    constexpr unsigned int PER = MLM_CROP_SLOTS_PER_CHUNK / MLM_BLOCK;
    __shared__ unsigned long long s_wave[MLM_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const unsigned long long i0 = (unsigned long long)c * MLM_CROP_SLOTS_PER_CHUNK + (unsigned long long)threadIdx.x * PER;
        unsigned long long mine = 0;
        for (unsigned int k = 0; k < PER; ++k)
            if (i0 + k < n) mine += row[i0 + k].units;
        unsigned long long incl = mine; // inclusive scan over the wave's lanes
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        __syncthreads(); // (the previous chunk's wave totals are read)
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long at = chunk_sum[(size_t)c * MLM_PACK_COLS] + incl - mine;
        for (int w = 0; w < wave; ++w) at += s_wave[w];
        for (unsigned int k = 0; k < PER; ++k)
            if (i0 + k < n) {
                off[i0 + k] = at;
                at += row[i0 + k].units;
            }
    }
}

__global__ void k_pack_head(uint8_t *__restrict__ stream, const MlmPackHeader H) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint8_t b[MLM_PACK_HEADER];
    mlm_pack_header_write(H, b);
    for (int i = 0; i < MLM_PACK_HEADER / 4; ++i) ((uint32_t *)stream)[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
}

__global__ __launch_bounds__(MLM_BLOCK) void k_pack_write(const MlmDev P, const MlmPack K) {
    const int lane = threadIdx.x & 63;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64), r1 = K.r1;
    const uint32_t W = K.W;
    const MlmPackRow *const rows = K.row;
    const unsigned long long *const off = K.off;
    const unsigned long long base_units = K.base_units, below = lane ? ~0ull >> (64 - lane) : 0ull;
    uint8_t *const stream = K.stream;
    for (unsigned int r = K.r0 + blockIdx.x * (MLM_BLOCK / 64) + wave; r < r1; r += waves) {
        MlmPackSrc R;
        if (!mlm_pack_source(P, K, r, R)) continue; // (wave-uniform)
        const MlmPackRow row = rows[r];
        if (row.err || !row.pad0) continue; // (never: the host stops at a bad row)
        const unsigned long long o = base_units + off[r];
        uint8_t *const rec = stream + 8ull * o;
        uint32_t *const dir = (uint32_t *)(stream + MLM_PACK_HEADER + MLM_PACK_DIR * (unsigned long long)r);
        if (lane < 3) dir[lane] = (uint32_t)R.key[lane];
        if (lane == 3) dir[3] = (uint32_t)o;
        if (lane == 4) ((uint32_t *)rec)[0] = row.presence;
        if (lane == 5) ((uint32_t *)rec)[1] = row.n_lit;
        const uint32_t pres = row.presence & 63u, n_lit = row.n_lit;
        unsigned long long *const planes = (unsigned long long *)(rec + 8);
        uint32_t *const lits = (uint32_t *)(rec + 8 + 8ull * W * (unsigned long long)__builtin_popcount(pres));
        const bool my_plane = lane < 6 && (pres >> lane & 1u);
        const size_t my_at = (size_t)__builtin_popcount(pres & ((1u << (lane & 7)) - 1u)) * W;
        uint32_t base = 0;
        for (uint32_t j = 0; j < W; ++j) {
            uint32_t bits, co, ci, cv;
            mlm_pack_cell(R, K, 64u * j + (uint32_t)lane, bits, co, ci, cv);
            const unsigned long long b0 = __ballot(co & 1u), b1 = __ballot(co & 2u), b2 = __ballot(ci & 1u), b3 = __ballot(ci & 2u), b4 = __ballot(cv & 1u),
                                     b5 = __ballot(cv & 2u);
            if (my_plane) planes[my_at + j] = lane == 0 ? b0 : lane == 1 ? b1 : lane == 2 ? b2 : lane == 3 ? b3 : lane == 4 ? b4 : b5;
            const unsigned long long lit = b4 & b5;
            const uint32_t rank = base + (uint32_t)__builtin_popcountll(lit & below);
            if (cv == 3u && rank < n_lit) lits[rank] = bits;
            base += (uint32_t)__builtin_popcountll(lit);
        }
        if ((n_lit & 1u) && lane == 0) lits[n_lit] = 0u; // (the padding to 8 bytes)
    }
}

struct MlmUnpack {
    const uint8_t *s;         // the stream; [0, total) may be read
    unsigned long long total;
    uint32_t n, C, W, min_bits, max_bits;
    MlmPackRow *row;          // [n] the validator's answer
    uint32_t *next_err;       // [n] zeroed; block i - 1 writes what it finds wrong with block i's offset
    unsigned int r0, r1;      // the rows of this launch (the writer)
    int32_t *keys;            // the outputs, starting at row r0 (any may be null)
    float *lo;
    uint8_t *occ, *infl;
};

__global__ __launch_bounds__(MLM_BLOCK) void k_unpack_check(const MlmUnpack U) {
    const int lane = threadIdx.x & 63;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64);
    const uint8_t *const s = U.s;
    const unsigned long long total = U.total;
    const uint32_t n = U.n, C = U.C, W = U.W;
    for (unsigned int i = blockIdx.x * (MLM_BLOCK / 64) + wave; i < n; i += waves) {
        unsigned long long o, size;
        uint32_t pres, n_lit;
        const int opened = mlm_pack_block_open(s, total, W, n, i, o, pres, n_lit, size); // (wave-uniform)
        uint32_t flags = 0, c_lit = 0, c_min = 0, c_max = 0;
        if (opened == 0)
            for (uint32_t j = (uint32_t)lane; j < W; j += 64u) {
                unsigned long long w[6];
                mlm_pack_block_words(s, o, W, pres, j, w);
                flags |= mlm_pack_word_check(w, C, j, c_lit, c_min, c_max);
            }
        flags = (__ballot(flags & 1u) ? 1u : 0u) | (__ballot(flags & 2u) ? 2u : 0u);
        for (int off = 32; off > 0; off >>= 1) c_lit += __shfl_down(c_lit, off), c_min += __shfl_down(c_min, off), c_max += __shfl_down(c_max, off);
        c_lit = __shfl(c_lit, 0);
        int next = 0;
        const int own = mlm_pack_block_close(s, total, n, i, opened, o, size, flags, n_lit, c_lit, next);
        if (lane == 0) {
            MlmPackRow out{};
            out.units = (uint32_t)(size / 8ull), out.n_lit = c_lit, out.n_min = c_min, out.n_max = c_max, out.presence = pres, out.err = (uint32_t)own, out.pad0 = 1u;
            U.row[i] = out;
            if (i + 1u < n) U.next_err[i + 1u] = (uint32_t)next;
        }
    }
}

__global__ __launch_bounds__(MLM_BLOCK) void k_unpack_write(const MlmUnpack U) {
    const int lane = threadIdx.x & 63;
    const unsigned int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned int waves = gridDim.x * (MLM_BLOCK / 64), r1 = U.r1;
    const uint8_t *const s = U.s;
    const unsigned long long total = U.total, below = lane ? ~0ull >> (64 - lane) : 0ull;
    const uint32_t n = U.n, C = U.C, W = U.W, min_bits = U.min_bits, max_bits = U.max_bits;
    for (unsigned int i = U.r0 + blockIdx.x * (MLM_BLOCK / 64) + wave; i < r1; i += waves) {
        unsigned long long o, size;
        uint32_t pres, n_lit;
        const int opened = mlm_pack_block_open(s, total, W, n, i, o, pres, n_lit, size);
        if (opened != 0) continue; // (never: the stream was validated; the record lies inside the total)
        const size_t at = (size_t)(i - U.r0);
        if (U.keys && lane < 3) U.keys[3 * at + lane] = (int32_t)mlm_pack_u32(s + MLM_PACK_HEADER + MLM_PACK_DIR * (unsigned long long)i + 4 * lane);
        const uint8_t *const lits = s + 8ull * o + 8ull + 8ull * W * (unsigned long long)__builtin_popcount(pres);
        uint32_t base = 0;
        for (uint32_t j = 0; j < W; ++j) {
            unsigned long long w[6];
            mlm_pack_block_words(s, o, W, pres, j, w);
            const unsigned long long lit = w[4] & w[5];
            const uint32_t c = 64u * j + (uint32_t)lane;
            if (c < C) {
                const uint32_t co = (uint32_t)(w[0] >> lane & 1ull) | (uint32_t)(w[1] >> lane & 1ull) << 1, ci = (uint32_t)(w[2] >> lane & 1ull) | (uint32_t)(w[3] >> lane & 1ull) << 1,
                               cv = (uint32_t)(w[4] >> lane & 1ull) | (uint32_t)(w[5] >> lane & 1ull) << 1;
                const uint32_t rank = base + (uint32_t)__builtin_popcountll(lit & below);
                const uint32_t literal = cv == 3u && rank < n_lit ? mlm_pack_u32(lits + 4ull * rank) : 0u;
                if (U.lo) ((uint32_t *)U.lo)[at * C + c] = mlm_pack_val_bits(cv, min_bits, max_bits, literal);
                if (U.occ) U.occ[at * C + c] = mlm_pack_class_byte(co);
                if (U.infl) U.infl[at * C + c] = mlm_pack_class_byte(ci);
            }
            base += (uint32_t)__builtin_popcountll(lit);
        }
    }
}
