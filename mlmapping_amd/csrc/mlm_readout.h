// mlm_readout.h — host part of mlmap_hip.hip (included after mlm_mirror.h): what the read-outs (mlm_export_window .. mlm_export_clusters,
// mlm_query_rays .. mlm_query_views, mlm_render_depth) share on the host.  The box check, the brick cover and the staging layout
// themselves are pure arithmetic (mlm_host.h), as are the tile walk (mlm_for_tiles) and the rows of a staged round (mlm_stage_rows);
// here they meet the handle, device memory and the stream: kept buffers (readout_reserve), the pinned control block (ctrl_block,
// read_back), the channels of a call (ReadoutChannels) and the loops over their ranges (chunk_rounds, for_chunks, page_rounds).
#pragma once

namespace {
constexpr unsigned int kEsdfMaskGrid = 2048, kEsdfPassGrid = 4096;
constexpr unsigned int kGridColGrid = 1u << 16; // most workgroups of k_grid_columns (a brick stack each, grid-stride)
constexpr unsigned int kReachGrid = 1u << 16; // most workgroups of the mlm_export_reach kernels (grid-stride loops over voxels / tiles)

// mlm_box_check with the entry point's error text
int box_check(mlm_handle *h, const char *what, const int32_t lo[3], const int32_t dims[3], long long D[3], long long &nvox) {
    const int bad = mlm_box_check(lo, dims, D, nvox);
    if (!bad) return MLM_OK;
    h->err = std::string(what) + (bad == 1 ? ": dims must be >= 1 and lo + dims must fit an int32" : ": more than 2^31 - 1 voxels");
    return MLM_ERR_INVALID;
}

// mlm_brick_cover of the first `axes` axes of a box, into the b0 / nb of a kernel's parameters
template <class L, class D> void brick_cover(const mlm_handle *h, int axes, const L *lo, const D *d, long long *b0, int *nb) {
    for (int a = 0; a < axes; ++a) mlm_brick_cover(h->P.n, lo[a], d[a], b0[a], nb[a]);
}

// one wave per item, four to a workgroup; at most `cap` workgroups (the kernel strides over the rest)
inline unsigned int wave_grid(size_t m, unsigned int cap = ~0u) {
    return std::min<unsigned int>((unsigned int)((m + MLM_BLOCK / 64 - 1) / (MLM_BLOCK / 64)), cap);
}

// device memory this device's kernels use in place; anything else (pageable, pinned or managed host memory) is staged
bool readout_in_place(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // (pageable host memory is unknown to the runtime)
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

// a kept buffer of at least `bytes`; a failed allocation leaves the handle as it was, minus the old buffer
int readout_reserve(mlm_handle *h, KeptBuf &kept, size_t bytes, const char *what) {
    if (bytes <= kept.bytes) return MLM_OK;
    dev_free(h, kept.p, kept.bytes);
    kept = KeptBuf{};
    void *v = nullptr;
    if (hipMalloc(&v, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->err = std::string(what) + ": no device memory for " + std::to_string(bytes >> 20) + " MB of scratch";
        return MLM_ERR_CAPACITY;
    }
    h->alloc_bytes += bytes;
    h->allocs.push_back(v);
    kept = KeptBuf{v, bytes};
    return MLM_OK;
}

// the handle's pinned control block, allocated on first use
int ctrl_block(mlm_handle *h) {
    if (!h->h_ctrl) HIPCHK(h, hipHostMalloc((void **)&h->h_ctrl, sizeof(MlmCtrlBlock), hipHostMallocDefault));
    return MLM_OK;
}

// Waits for the stream; ahead of that, n 32- or 64-bit words of device memory are copied into the pinned control block, where `got`
// then points at them (n == 0: only the wait, `got` is null).
template <class T> int read_back(mlm_handle *h, const T *dev, size_t n, const T *&got) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "control words and counters");
    got = nullptr;
    if (n) {
        if (n * sizeof(T) > sizeof(MlmCtrlBlock::words)) return MLM_ERR_INVALID; // (no caller asks for that many)
        if (int rc = ctrl_block(h)) return rc;
        got = reinterpret_cast<const T *>(&h->h_ctrl->words);
        HIPCHK(h, hipMemcpyAsync(&h->h_ctrl->words, dev, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}
// ... n counters, widened into the int64 of a summary
int read_back(mlm_handle *h, const unsigned long long *dev, size_t n, int64_t *out) {
    const unsigned long long *got;
    if (int rc = read_back(h, dev, n, got)) return rc;
    for (size_t i = 0; i < n; ++i) out[i] = (int64_t)got[i];
    return MLM_OK;
}

// The channels of a read-out: its input and output arrays, each with its bytes per element.  A channel in device memory is used
// in place; one in host memory is staged, range by range (a tile, a chunk of a batch), through one kept buffer of the handle
// that all staged channels share (mlm_stage_layout): d_win_stage for the exports, copied with hipMemcpyDefault, d_ray_stage for
// the queries, copied with directed kinds.
struct ReadoutChan {
    const void *ptr;
    size_t elem;
};
template <int N> struct ReadoutChannels {
    void *ptr[N];
    size_t elem[N], off[N];
    bool present[N], staged[N];
    bool any_staged = false, all_host = true; // all_host: no channel in device memory (the host mirror may answer)
    KeptBuf &buf;
    const bool directed;

    ReadoutChannels(KeptBuf &kept, const ReadoutChan (&ch)[N], bool directed_copies = false) : buf(kept), directed(directed_copies) {
        for (int c = 0; c < N; ++c) {
            ptr[c] = const_cast<void *>(ch[c].ptr);
            elem[c] = ch[c].elem;
            off[c] = 0;
            present[c] = ptr[c] != nullptr;
            staged[c] = present[c] && !readout_in_place(ptr[c]);
            any_staged |= staged[c];
            all_host = all_host && (staged[c] || !present[c]);
        }
    }
    // room for `count[c]` elements of every staged channel
    int reserve(mlm_handle *h, const char *what, const size_t (&count)[N]) {
        const size_t bytes = mlm_stage_layout(N, present, staged, elem, count, off);
        return bytes ? readout_reserve(h, buf, bytes, what) : MLM_OK;
    }
    // ... the same count for all of them
    int reserve(mlm_handle *h, const char *what, size_t count) {
        size_t counts[N];
        std::fill(counts, counts + N, count);
        return reserve(h, what, counts);
    }
    // where a kernel reads or writes the range of channel c that starts at element i0: null, the staging, or the caller's memory
    void *at(int c, size_t i0) const {
        return !present[c] ? nullptr : staged[c] ? (void *)((char *)buf.p + off[c]) : (void *)((char *)ptr[c] + i0 * elem[c]);
    }
    // the staged ones of channels [c0, c1): m elements from i0 of the caller's memory into the staging, or back
    int copy_in(mlm_handle *h, int c0, int c1, size_t i0, size_t m) {
        for (int c = c0; c < c1; ++c)
            if (staged[c])
                HIPCHK(h, hipMemcpyAsync(at(c, i0), (const char *)ptr[c] + i0 * elem[c], m * elem[c], directed ? hipMemcpyHostToDevice : hipMemcpyDefault,
                                         h->stream));
        return MLM_OK;
    }
    int copy_out(mlm_handle *h, int c0, int c1, size_t i0, size_t m) {
        for (int c = c0; c < c1; ++c)
            if (staged[c])
                HIPCHK(h, hipMemcpyAsync((char *)ptr[c] + i0 * elem[c], at(c, i0), m * elem[c], directed ? hipMemcpyDeviceToHost : hipMemcpyDefault,
                                         h->stream));
        return MLM_OK;
    }
    // the staged bytes of one element of every channel
    size_t staged_elem_bytes() const {
        size_t b = 0;
        for (int c = 0; c < N; ++c) b += staged[c] ? elem[c] : 0;
        return b;
    }
};

// The elements [0, n) of a channel set in ranges of `chunk`: the input channels [in0, in1) of the range copied in, launch(i0, m, at)
// — at[c]: where a kernel finds channel c's range of m elements from i0 — checked, the output channels [out0, out1) copied out.
// Nothing waits: the stream orders the rounds' use of the staging.  launch returns MLM_OK, or the error that ends the call.
template <int N, class F> int chunk_rounds(mlm_handle *h, ReadoutChannels<N> &ch, size_t n, size_t chunk, int in0, int in1, int out0, int out1, F launch) {
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        void *at[N];
        for (int c = 0; c < N; ++c) at[c] = ch.at(c, i0);
        if (int rc = ch.copy_in(h, in0, in1, i0, m)) return rc;
        if (int rc = launch(i0, m, at)) return rc;
        HIPCHK(h, hipGetLastError());
        if (int rc = ch.copy_out(h, out0, out1, i0, m)) return rc;
    }
    return MLM_OK;
}
// ... a whole batched query behind its drain: the staging reserved for a chunk, the rounds, the wait
template <int N, class F>
int for_chunks(mlm_handle *h, ReadoutChannels<N> &ch, const char *what, size_t n, size_t chunk, int in0, int in1, int out0, int out1, F launch) {
    if (int rc = ch.reserve(h, what, chunk)) return rc;
    if (int rc = chunk_rounds(h, ch, n, chunk, in0, in1, out0, out1, launch)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

// Rows of blocks paged out through the exports' staging (mlm_crop_blocks, mlm_warp_blocks): the rows of a round (mlm_stage_rows with
// kCropStageBytes and the knob "crop_stage_rows"), and the rounds — launch(r0, r1), all channels copied out and, where anything
// is staged, a wait per round.
constexpr size_t kCropStageBytes = 64u << 20; // staged rows of a page-out into host memory, per round
template <int N> size_t page_rows(const ReadoutChannels<N> &ch, size_t n) {
    long long kv = 0;
    if (!knob("crop_stage_rows", kv)) kv = 0; // (test knob: rounds of a few rows)
    return mlm_stage_rows(n, ch.staged_elem_bytes(), kCropStageBytes, kv);
}
template <int N, class F> int page_rounds(mlm_handle *h, ReadoutChannels<N> &ch, size_t n, size_t rows, F launch) {
    for (size_t r0 = 0; r0 < n; r0 += rows) {
        const size_t r1 = std::min(n, r0 + rows);
        launch(r0, r1);
        HIPCHK(h, hipGetLastError());
        if (ch.any_staged) {
            if (int rc = ch.copy_out(h, 0, N, r0, r1 - r0)) return rc;
            HIPCHK(h, hipStreamSynchronize(h->stream)); // (the staging is reused by the next round)
        }
    }
    return MLM_OK;
}

// A small batch whose arrays are all host memory, answered from the host mirror (mlm_mirror.h) as run_query answers its small
// batches.  1: `answer()` has answered it; 0: not wanted, or no mirror (no pinned host memory for it, or more than its limit
// allows: this and all later batches run as kernels); < 0: an error of the frames in flight, reported by the drain.
template <class F> int mirror_try(mlm_handle *h, bool wanted, int n, F answer) {
    if (!wanted) return 0;
    const int rc = mirror_sync(h);
    if (rc == MLM_OK) {
        answer();
        h->mir.n_host_queries += n;
        return 1;
    }
    return !h->mir.alloc_failed && rc != kMirrorUnavailable ? rc : 0;
}

// the mask and the three passes of one tile of mlm_export_esdf (mlm_kernels_esdf.h) into fa [ez][ey][ex]; T: u16 (unsigned) or
// u16x2 (signed)
template <bool SIGNED>
void esdf_passes(mlm_handle *h, const MlmEsdf &E, int C, uint8_t *mask, void *fa, void *fb, int ex, int ey, int ez) {
    using T = typename std::conditional<SIGNED, mlm_u16x2, uint16_t>::type;
    launch(h, k_esdf_mask, bricks_grid((long long)E.nb[0] * E.nb[1] * E.nb[2], kEsdfMaskGrid), 0, h->P, E);
    // x: mask [gd2 * gd1][gd0] -> fa [gd2 * gd1][ex]
    const long long rows = (long long)E.gd[2] * E.gd[1], xtasks = rows * ((ex + 63) / 64);
    launch(h, k_esdf_x<SIGNED>, bricks_grid((xtasks + 3) / 4, kEsdfPassGrid), 0, mask, fa, rows, E.gd[0], ex, C);
    // y: fa [gd2][gd1][ex] -> fb [gd2][ey][ex];  z: fb [gd2][ey * ex] -> fa [ez][ey * ex]
    const int TLmax = SIGNED ? MLM_ESDF_LINE_TL / 2 : MLM_ESDF_LINE_TL;
    auto line = [&](const void *in, void *out, long long X, int Lout, int outer) {
        const int lc = (Lout + TLmax - 1) / TLmax, TL = (Lout + lc - 1) / lc; // (rows spread evenly over the line chunks)
        const long long tiles = (long long)outer * lc * ((X + 63) / 64);
        const size_t lds = (size_t)(TL + 2 * C - 2) * 64 * sizeof(T);
        hipLaunchKernelGGL(k_esdf_line<T>, dim3((unsigned int)std::min<long long>(tiles, kEsdfPassGrid)), dim3(MLM_BLOCK), lds, h->stream,
                           (const T *)in, (T *)out, X, Lout, outer, C, TL);
    };
    line(fa, fb, ex, ey, E.gd[2]);
    line(fb, fa, (long long)ey * ex, ez, 1);
}

// the passes and the outputs of one tile of mlm_export_esdf
template <bool SIGNED>
void esdf_tile(mlm_handle *h, const MlmEsdf &E, int C, uint8_t *mask, void *fa, void *fb, const MlmEsdfOut &Q) {
    esdf_passes<SIGNED>(h, E, C, mask, fa, fb, Q.fd[0], Q.fd[1], Q.fd[2]);
    const long long nt = (long long)Q.td[0] * Q.td[1] * Q.td[2];
    launch(h, k_esdf_out<SIGNED>, lanes_grid((size_t)nt, kEsdfPassGrid), 0, (const void *)fa, Q);
}

// the class mask of a whole box (k_esdf_mask with no growth) into out [dims2][dims1][dims0]
void mask_box(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, uint8_t *out) {
    MlmEsdf E{};
    for (int a = 0; a < 3; ++a) {
        E.glo[a] = lo[a];
        E.gd[a] = dims[a];
    }
    brick_cover(h, 3, E.glo, E.gd, E.b0, E.nb);
    E.flags = flags;
    E.mask = out;
    launch(h, k_esdf_mask, bricks_grid((long long)E.nb[0] * E.nb[1] * E.nb[2], kEsdfMaskGrid), 0, h->P, E);
}

// D_out of mlm_export_esdf at max_dist = C over the box [lo, lo + D), unsigned, tile by tile (mlm_esdf_plan without a staging cap;
// each tile a contiguous range of the box): per_tile(fa, j0, nt) turns the tile's u16 field fa into the nt bytes of the box from
// voxel j0 on (a launch on h->stream).  Scratch as mlm_export_esdf's.
template <class F> int esdf_tiles(mlm_handle *h, const char *what, const int32_t lo[3], const long long D[3], int C, int flags, F per_tile) {
    long long box_cap = kEsdfBoxVoxels, kv;
    if (knob("esdf_tile_vox", kv)) box_cap = kv;
    const MlmEsdfPlan ep = mlm_esdf_plan(D, C, false, box_cap, 1ll << 62);
    if (ep.T[0] < 1) { // (not with the caps mlm_debug_set admits)
        h->err = std::string(what) + ": no ESDF tile fits the voxel cap";
        return MLM_ERR_INVALID;
    }
    const size_t mask_bytes = mlm_align256((size_t)ep.grown), field_bytes = mlm_align256((size_t)ep.grown * 2);
    if (int rc = readout_reserve(h, h->d_esdf_scratch, mask_bytes + 2 * field_bytes, what)) return rc;
    uint8_t *emask = (uint8_t *)h->d_esdf_scratch.p;
    void *fa = emask + mask_bytes, *fb = emask + mask_bytes + field_bytes;
    return mlm_for_tiles(D, ep.T, [&](const long long org[3], const int td[3], long long out_base) -> int {
        MlmEsdf E{};
        for (int a = 0; a < 3; ++a) {
            E.glo[a] = lo[a] + org[a] - ep.H;
            E.gd[a] = td[a] + (int)(2 * ep.H);
        }
        brick_cover(h, 3, E.glo, E.gd, E.b0, E.nb);
        E.flags = flags;
        E.mask = emask;
        esdf_passes<false>(h, E, C, emask, fa, fb, td[0], td[1], td[2]);
        per_tile((const uint16_t *)fa, out_base, (long long)td[0] * td[1] * td[2]);
        HIPCHK(h, hipGetLastError());
        return MLM_OK;
    });
}

// Sweeps of a field over a tiled box (mlm_export_reach, mlm_export_route) in groups of `group`: launch_sweep(s, word) enqueues sweep
// s, which sets *word when it marks something.  After each group the host reads the group's words (read_back) and stops
// at the first sweep that marked nothing: the sweeps enqueued behind it found no dirty tile.  Returns the sweeps needed, or an error
// (< 0).
template <class F> long long settle(mlm_handle *h, const char *what, long long cap, long long group, unsigned int *marked, F launch_sweep) {
    long long sweeps = 0, needed = -1;
    while (needed < 0) {
        if (sweeps >= cap) { // (mlm_reach.h, mlm_route.h: cannot happen; an endless loop otherwise)
            h->err = std::string(what) + ": the field did not settle within " + std::to_string(sweeps) + " sweeps";
            return MLM_ERR_HIP;
        }
        if (sweeps) HIPCHK(h, hipMemsetAsync(marked, 0, (size_t)group * sizeof(unsigned int), h->stream));
        for (long long g = 0; g < group; ++g, ++sweeps) launch_sweep(sweeps, marked + g);
        HIPCHK(h, hipGetLastError());
        const unsigned int *got;
        if (int rc = read_back(h, (const unsigned int *)marked, (size_t)group, got)) return rc;
        for (long long g = 0; g < group && needed < 0; ++g)
            if (got[g] == 0) needed = sweeps - group + g + 1;
    }
    return needed;
}

// ... and the end of such a call: waits for its outputs, and fills the summary from the three counters the output kernel left at
// cnt (the third less one) and the sweeps needed
int settle_finish(mlm_handle *h, const unsigned long long *cnt, long long needed, int64_t summary[4]) {
    if (int rc = read_back(h, cnt, summary ? 3 : 0, summary)) return rc;
    if (summary) {
        summary[2] -= 1;
        summary[3] = (int64_t)needed;
    }
    return MLM_OK;
}

} // namespace
