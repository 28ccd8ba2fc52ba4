// mlm_pack_host.h — host part of mlmap_hip.hip (included behind mlm_delta_host.h): the drivers of mlm_pack_blocks and
// mlm_unpack_blocks.  The rule is mlm_pack.h's, the kernels are mlm_kernels_pack.h's.
//
// Order of a pack: the handle's scratch and the staging of host rows reserved; for the live map the selection and the sort; pass 1 (host
// rows copied in round by round), the chunk sums, the scan, the offsets; the host reads the eight totals once (the call's one
// synchronisation ahead of its output), reports a bad byte, fills the summary, checks the capacity; then — behind every check and
// every allocation — the header and pass 2 (host rows copied in again), and a staged stream copied out.
// Order of an unpack: the header read and checked on the host; a host stream staged whole; the validator, the chunk sums, the scan;
// the host reads the totals, reports the verdict, checks the cap; then the outputs' staging reserved and the rows written in rounds.
#pragma once

namespace {
static_assert(MLM_PACK_DRY == MLM_PACK_F_DRY && MLM_PACK_NO_INFL == MLM_PACK_F_NO_INFL && MLM_PACK_ROW == MLM_PACK_SUMS,
              "mlm_pack.h restates the constants of include/mlmap_hip.h");
static_assert(sizeof(MlmPackRow) == 32, "a row of pass 1 is two 16-byte stores");

constexpr unsigned int kPackGrid = 4096; // most workgroups of the pack and unpack kernels (knob "pack_grid"): a wave takes several rows

unsigned int pack_grid_cap() {
    long long kv = 0;
    return knob("pack_grid", kv) ? (unsigned int)kv : kPackGrid;
}

// the scratch of both calls: rows | offsets (pack) or successor verdicts (unpack) | chunk sums | totals | `extra` bytes
struct PackScratch {
    MlmPackRow *row;
    unsigned long long *off, *chunk_sum, *totals;
    char *extra;
    unsigned int chunks;
};
int pack_scratch(mlm_handle *h, const char *what, unsigned int N, size_t extra, PackScratch &X) {
    X.chunks = (N + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
    const size_t o_off = mlm_align256((size_t)N * sizeof(MlmPackRow)), o_ch = o_off + mlm_align256((size_t)N * 8),
                 o_tot = o_ch + mlm_align256((size_t)X.chunks * MLM_PACK_COLS * 8), o_extra = o_tot + 256;
    if (int rc = readout_reserve(h, h->d_pack, o_extra + extra, what)) return rc;
    char *b = (char *)h->d_pack.p;
    X.row = (MlmPackRow *)b, X.off = (unsigned long long *)(b + o_off), X.chunk_sum = (unsigned long long *)(b + o_ch), X.totals = (unsigned long long *)(b + o_tot);
    X.extra = b + o_extra;
    return MLM_OK;
}
// the chunk sums and the scan over the rows; next_err: the validator's
void pack_sums(mlm_handle *h, const PackScratch &X, unsigned int N, const uint32_t *next_err) {
    if (X.chunks) launch(h, k_pack_chunks, std::min(X.chunks, kCropGrid), 0, (const MlmPackRow *)X.row, next_err, N, X.chunks, X.chunk_sum);
    launch(h, k_pack_scan, 1u, 0, X.chunk_sum, X.chunks, X.totals);
}

// everything of mlm_pack_blocks behind the argument check and the drain
int pack_run(mlm_handle *h, const MlmAgeSel &S, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl, int flags, size_t cap_bytes,
             void *stream, bool stream_dev, int64_t *summary) {
    const char *const what = "mlm_pack_blocks";
    int64_t sum[MLM_PACK_ROW] = {};
    auto report = [&]() {
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    const bool live = keys == nullptr;
    int rc = MLM_OK;
    unsigned int nb = 0;
    if (live) {
        if ((rc = read_global(h))) return rc;
        nb = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks);
    }
    const unsigned int N = live ? nb : (unsigned int)n; // rows of pass 1 (live: sorted positions, the selected ones in front)
    const uint32_t C = (uint32_t)h->P.cells, W = mlm_pack_words(C);
    const unsigned int grid_cap = pack_grid_cap();
    const size_t sort_bytes = live && nb ? mlm_sort_temp_bytes(nb) : 0, b8 = mlm_align256((size_t)nb * 8), b4 = mlm_align256((size_t)nb * 4);
    PackScratch X{};
    if ((rc = pack_scratch(h, what, N, live ? 2 * b8 + 2 * b4 + mlm_align256(sort_bytes) : 0, X))) return rc;
    // host rows go through the queries' staging, a round of rows at a time (the stream's staging is the exports': reserved later, and
    // must not move this one)
    ReadoutChannels<4> in(h->d_ray_stage, {{keys, 3 * sizeof(int32_t)}, {log_odds, (size_t)C * sizeof(float)}, {occ, (size_t)C}, {infl, (size_t)C}});
    const size_t page = live || !N ? 0 : page_rows(in, N);
    if (page && (rc = in.reserve(h, what, page))) return rc;

    MlmPack K{};
    K.nb = nb, K.n = N, K.C = C, K.W = W, K.min_bits = mlm_fuse_bits(h->P.lo_min), K.max_bits = mlm_fuse_bits(h->P.lo_max);
    K.no_infl = (flags & MLM_PACK_NO_INFL) ? 1 : 0;
    K.row = X.row, K.off = X.off;
    if (live && nb) {
        unsigned long long *packed = (unsigned long long *)X.extra, *sorted = (unsigned long long *)(X.extra + b8);
        uint32_t *slot_of = (uint32_t *)(X.extra + 2 * b8), *sorted_slot = (uint32_t *)(X.extra + 2 * b8 + b4);
        launch(h, k_pack_select, lanes_grid(nb, kCropGrid), 0, h->P, S, nb, packed, slot_of);
        HIPCHK(h, hipGetLastError());
        if (mlm_sort_pairs_u64_u32(X.extra + 2 * b8 + 2 * b4, sort_bytes, packed, sorted, slot_of, sorted_slot, nb, h->stream) != 0) {
            (void)hipStreamSynchronize(h->stream);
            h->err = std::string(what) + ": the sort of the packed keys failed";
            return MLM_ERR_HIP;
        }
        K.sorted = sorted, K.sorted_slot = sorted_slot;
    }
    // a pass over the rows: the live map in one launch, a dump in rounds of `page` rows
    auto pass = [&](auto kernel) -> int {
        if (live) {
            K.r0 = 0, K.r1 = N;
            if (N) launch(h, kernel, wave_grid(N, grid_cap), 0, h->P, K);
            return MLM_OK;
        }
        for (size_t r0 = 0; r0 < N; r0 += page) {
            const size_t m = std::min(page, (size_t)N - r0);
            if (int e = in.copy_in(h, 0, 4, r0, m)) return e;
            K.keys = (const int32_t *)in.at(0, r0), K.lo = (const float *)in.at(1, r0), K.occ = (const uint8_t *)in.at(2, r0), K.infl = (const uint8_t *)in.at(3, r0);
            K.r0 = (unsigned int)r0, K.r1 = (unsigned int)(r0 + m);
            launch(h, kernel, wave_grid(m, grid_cap), 0, h->P, K);
        }
        return MLM_OK;
    };
    if ((rc = pass(k_pack_size))) return rc;
    pack_sums(h, X, N, nullptr);
    if (X.chunks) launch(h, k_pack_offsets, std::min(X.chunks, kCropGrid), 0, (const MlmPackRow *)X.row, N, X.chunks, (const unsigned long long *)X.chunk_sum, X.off);
    HIPCHK(h, hipGetLastError());
    const unsigned long long *got;
    if ((rc = read_back(h, (const unsigned long long *)X.totals, MLM_PACK_COLS, got))) return rc;
    if (got[6] != ~0ull) {
        h->err = std::string(what) + ": " + mlm_pack_check_text(9) + " (row " + std::to_string(got[6] >> 8) + ")";
        return MLM_ERR_INVALID;
    }
    const unsigned long long units = got[0], rows = got[1], front = mlm_pack_front_bytes(rows), total = front + 8ull * units;
    if (rows > N) {
        h->err = std::string(what) + ": the counts of pass 1 are inconsistent";
        return MLM_ERR_HIP;
    }
    sum[0] = (int64_t)rows, sum[1] = (int64_t)total, sum[2] = (int64_t)mlm_pack_raw_bytes(rows, C), sum[3] = (int64_t)got[2], sum[4] = (int64_t)got[3], sum[5] = (int64_t)got[4],
    sum[6] = (int64_t)got[5];
    const bool writes = stream && !(flags & MLM_PACK_DRY);
    if (front / 8ull + units > MLM_PACK_MAX_UNITS) {
        h->err = std::string(what) + ": the stream of " + std::to_string(total) + " bytes does not fit 2^32 - 1 eight-byte units";
        report();
        return MLM_ERR_CAPACITY;
    }
    if (writes && total > (unsigned long long)cap_bytes) {
        h->err = std::string(what) + ": " + std::to_string(total) + " bytes would be written, the stream holds " + std::to_string(cap_bytes);
        report();
        return MLM_ERR_CAPACITY;
    }
    if (!writes) {
        report();
        return MLM_OK;
    }
    // every allocation before the first write: a host stream is staged whole
    if (!stream_dev && (rc = readout_reserve(h, h->d_win_stage, (size_t)total, what))) {
        report();
        return rc;
    }
    K.stream = stream_dev ? (uint8_t *)stream : (uint8_t *)h->d_win_stage.p;
    K.base_units = front / 8ull;
    MlmPackHeader H{C, (uint32_t)h->P.n, (uint32_t)rows, K.no_infl ? 1u : 0u, K.min_bits, K.max_bits, total, got[3]};
    launch(h, k_pack_head, 1u, 0, K.stream, H);
    if ((rc = pass(k_pack_write))) return rc;
    HIPCHK(h, hipGetLastError());
    if (!stream_dev) HIPCHK(h, hipMemcpyAsync(stream, K.stream, (size_t)total, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sum[7] = (int64_t)total;
    report();
    return MLM_OK;
}

// everything of mlm_unpack_blocks behind the argument check
int unpack_run(mlm_handle *h, const void *stream, size_t bytes, bool stream_dev, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, int64_t *summary) {
    const char *const what = "mlm_unpack_blocks";
    int64_t sum[MLM_PACK_ROW] = {};
    auto report = [&]() {
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    auto refuse = [&](int bad, const std::string &where) {
        h->err = std::string(what) + ": " + mlm_unpack_check_text(bad) + where;
        return MLM_ERR_INVALID;
    };
    int rc = MLM_OK;
    uint8_t head[MLM_PACK_HEADER] = {};
    if (bytes >= MLM_PACK_HEADER) {
        if (stream_dev) {
            if ((rc = ctrl_block(h))) return rc;
            HIPCHK(h, hipMemcpyAsync(&h->h_ctrl->words, stream, MLM_PACK_HEADER, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            std::memcpy(head, &h->h_ctrl->words, MLM_PACK_HEADER);
        } else {
            std::memcpy(head, stream, MLM_PACK_HEADER);
        }
    }
    const uint32_t C = (uint32_t)h->P.cells, W = mlm_pack_words(C);
    MlmPackHeader H{};
    if (const int bad = mlm_pack_header_check(head, bytes, C, (uint32_t)h->P.n, H)) return refuse(bad, "");
    const unsigned int N = H.n;
    PackScratch X{};
    if ((rc = pack_scratch(h, what, N, 0, X))) return rc;
    // a host stream goes through the queries' staging, whole: `total` bytes of it, no more
    if (!stream_dev) {
        if ((rc = readout_reserve(h, h->d_ray_stage, (size_t)H.total, what))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_ray_stage.p, stream, (size_t)H.total, hipMemcpyDefault, h->stream));
    }
    MlmUnpack U{};
    U.s = stream_dev ? (const uint8_t *)stream : (const uint8_t *)h->d_ray_stage.p;
    U.total = H.total, U.n = N, U.C = C, U.W = W, U.min_bits = H.min_bits, U.max_bits = H.max_bits;
    U.row = X.row, U.next_err = (uint32_t *)X.off;
    const unsigned int grid_cap = pack_grid_cap();
    if (N) {
        HIPCHK(h, hipMemsetAsync(U.next_err, 0, (size_t)N * 4, h->stream));
        launch(h, k_unpack_check, wave_grid(N, grid_cap), 0, U);
    }
    pack_sums(h, X, N, (const uint32_t *)U.next_err);
    HIPCHK(h, hipGetLastError());
    const unsigned long long *got;
    if ((rc = read_back(h, (const unsigned long long *)X.totals, MLM_PACK_COLS, got))) return rc;
    if (got[6] != ~0ull) return refuse((int)(got[6] & 0xFFull), " (block " + std::to_string(got[6] >> 8) + ")");
    sum[0] = N, sum[1] = (int64_t)H.total, sum[2] = (int64_t)mlm_pack_raw_bytes(N, C), sum[3] = (int64_t)got[2], sum[4] = (int64_t)got[3], sum[5] = (int64_t)got[4],
    sum[6] = (int64_t)got[5];
    const bool writes = keys || log_odds || occ || infl;
    if (writes && (unsigned int)cap < N) {
        h->err = std::string(what) + ": " + std::to_string(N) + " blocks would be written, the outputs hold " + std::to_string(cap);
        report();
        return MLM_ERR_CAPACITY;
    }
    if (!writes || !N) {
        report();
        return MLM_OK;
    }
    // every allocation before the first write: host outputs are staged in rounds through the exports' staging
    ReadoutChannels<4> ch(h->d_win_stage, {{keys, 3 * sizeof(int32_t)}, {log_odds, (size_t)C * sizeof(float)}, {occ, (size_t)C}, {infl, (size_t)C}});
    const size_t page = page_rows(ch, N);
    if ((rc = ch.reserve(h, what, page))) {
        report();
        return rc;
    }
    rc = page_rounds(h, ch, N, page, [&](size_t r0, size_t r1) {
        U.r0 = (unsigned int)r0, U.r1 = (unsigned int)r1;
        U.keys = (int32_t *)ch.at(0, r0), U.lo = (float *)ch.at(1, r0), U.occ = (uint8_t *)ch.at(2, r0), U.infl = (uint8_t *)ch.at(3, r0);
        launch(h, k_unpack_write, wave_grid(r1 - r0, grid_cap), 0, U);
    });
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sum[7] = (int64_t)N * (int64_t)((keys ? 12 : 0) + (log_odds ? 4 * (int64_t)C : 0) + (occ ? (int64_t)C : 0) + (infl ? (int64_t)C : 0));
    report();
    return MLM_OK;
}
} // namespace

int mlm_pack_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int n, const int32_t *keys, const float *log_odds, const uint8_t *occ,
                    const uint8_t *infl, int flags, size_t cap_bytes, void *stream, int64_t summary[MLM_PACK_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const bool stream_dev = stream && readout_in_place(stream);
    MlmAgeSel S{};
    if (const int bad = mlm_pack_check(key_lo, key_dims, n, keys, log_odds, occ, flags, stream_dev, (unsigned long long)(uintptr_t)stream, S)) {
        h->err = std::string("mlm_pack_blocks: ") + mlm_pack_check_text(bad);
        return MLM_ERR_INVALID;
    }
    const int rc = drain(h);
    if (rc) return rc;
    return pack_run(h, S, n, keys, log_odds, occ, infl, flags, cap_bytes, stream, stream_dev, summary);
}

int mlm_unpack_blocks(mlm_handle *h, const void *stream, size_t bytes, int flags, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl,
                      int64_t summary[MLM_PACK_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const bool stream_dev = stream && readout_in_place(stream);
    if (const int bad = mlm_unpack_check(stream, flags, cap, stream_dev, (unsigned long long)(uintptr_t)stream)) {
        h->err = std::string("mlm_unpack_blocks: ") + mlm_unpack_check_text(bad);
        return MLM_ERR_INVALID;
    }
    const int rc = drain(h);
    if (rc) return rc;
    return unpack_run(h, stream, bytes, stream_dev, cap, keys, log_odds, occ, infl, summary);
}
