// mlm_delta_host.h — host part of mlmap_hip.hip (included behind mlm_age_host.h): the driver of mlm_delta_blocks.  The rule is
// mlm_delta.h's, the kernels are mlm_kernels_delta.h's, the prefix is mlm_crop_blocks'.
//
// Order of a call: the handle's scratch and the staging of a host previous table reserved, the table copied; the digests, the sort,
// the join, the sums and the two ranked lists enqueued; the host reads the twelve sums and the control words once (the call's one
// synchronisation ahead of its outputs), reports a bad previous table, checks the three caps; then — behind every check and every
// allocation — the table rows, the gone keys and the emitted blocks written.  The call only reads the map.
#pragma once

namespace {
static_assert(MLM_DELTA_DRY == MLM_DELTA_F_DRY && MLM_DELTA_NO_INFL == MLM_DELTA_F_NO_INFL && MLM_DELTA_ROW == MLM_DELTA_SUMS,
              "mlm_delta.h restates the constants of include/mlmap_hip.h");

constexpr unsigned int kDeltaDigestGrid = 2048; // most workgroups of k_delta_digest (knob "delta_grid"): a wave takes several blocks

// everything of mlm_delta_blocks behind the argument check and the drain
int delta_run(mlm_handle *h, const MlmAgeSel &S, int n_prev, const int32_t *prev_keys, const uint64_t *prev_digest, int flags, int cap_table, int32_t *cur_keys,
              uint64_t *cur_digest, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, uint8_t *kind, int cap_gone, int32_t *gone_keys,
              int64_t *summary) {
    int64_t sum[MLM_DELTA_ROW] = {};
    auto report = [&]() {
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    int rc = read_global(h);
    if (rc) return rc;
    const unsigned int nb = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks), np = (unsigned int)n_prev;
    sum[0] = nb, sum[2] = np;
    if (nb == 0 && np == 0) {
        report();
        return MLM_OK;
    }
    const size_t C = (size_t)h->P.cells;
    long long kv = 0;
    const unsigned int grid_cap = knob("delta_grid", kv) ? (unsigned int)kv : kDeltaDigestGrid;
    const unsigned int dig_grid = nb ? wave_grid(nb, grid_cap) : 0u, join_grid = lanes_grid((size_t)nb + np, kCropGrid);
    // the handle's scratch: packed keys, twice | slots, twice | digests | kinds | emitted list | row states | gone list | chunk counts of
    // both prefixes | the twelve sums with the control words behind them | partial rows | the sort's scratch
    const unsigned int chunks_b = (nb + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK, chunks_p = (np + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
    const size_t sort_bytes = nb ? mlm_sort_temp_bytes(nb) : 0;
    const size_t b4 = mlm_align256((size_t)nb * 4), b8 = mlm_align256((size_t)nb * 8), p4 = mlm_align256((size_t)np * 4);
    const size_t o_kb = b8, o_va = 2 * b8, o_vb = o_va + b4, o_dg = o_vb + b4, o_kind = o_dg + 2 * b8, o_el = o_kind + b4, o_ps = o_el + b4, o_gl = o_ps + p4,
                 o_chb = o_gl + p4, o_chp = o_chb + mlm_align256((size_t)chunks_b * 4), o_ctrl = o_chp + mlm_align256((size_t)chunks_p * 4), o_part = o_ctrl + 256,
                 o_sort = o_part + mlm_align256(((size_t)dig_grid + join_grid) * MLM_DELTA_ROW * 8), total = o_sort + mlm_align256(sort_bytes);
    if ((rc = readout_reserve(h, h->d_delta, total, "mlm_delta_blocks"))) return rc;
    // a host previous table goes through the queries' staging (the outputs' staging is reserved later, and must not move it)
    ReadoutChannels<2> in(h->d_ray_stage, {{prev_keys, 3 * sizeof(int32_t)}, {prev_digest, 2 * sizeof(uint64_t)}});
    if (np && (rc = in.reserve(h, "mlm_delta_blocks", (size_t)np))) return rc;
    if (np && (rc = in.copy_in(h, 0, 2, 0, (size_t)np))) return rc;

    char *b = (char *)h->d_delta.p;
    MlmDelta D{};
    D.S = S, D.nb = nb, D.n_prev = np, D.no_infl = (flags & MLM_DELTA_NO_INFL) ? 1 : 0;
    D.prev_keys = np ? (const int32_t *)in.at(0, 0) : nullptr, D.prev_dg = np ? (const unsigned long long *)in.at(1, 0) : nullptr;
    D.packed = (unsigned long long *)b, D.sorted = (const unsigned long long *)(b + o_kb);
    D.slot_of = (uint32_t *)(b + o_va), D.sorted_slot = (const uint32_t *)(b + o_vb);
    D.dg = (unsigned long long *)(b + o_dg), D.kind = (uint32_t *)(b + o_kind), D.elist = (unsigned int *)(b + o_el);
    D.pstate = (uint32_t *)(b + o_ps), D.glist = (unsigned int *)(b + o_gl);
    D.part = (unsigned long long *)(b + o_part);
    unsigned int *chunk_b = (unsigned int *)(b + o_chb), *chunk_p = (unsigned int *)(b + o_chp);
    unsigned long long *sums = (unsigned long long *)(b + o_ctrl);
    unsigned int *ctrl = (unsigned int *)(sums + MLM_DELTA_ROW); // the thirteenth and fourteenth word of the read-back
    // four voxels per lane where a block's rows are aligned and fill a quarter of a wave at least, else one (as k_age_apply)
    const int fw = mlm_crop_float_width(h->P.cells), bw = mlm_crop_byte_width(h->P.cells);
    const int V = fw == 16 && bw >= 4 && h->P.cells >= 64 ? 4 : 1;

    HIPCHK(h, hipMemsetAsync(sums, 0, 256, h->stream));
    if (nb) {
        launch(h, V == 4 ? k_delta_digest<4> : k_delta_digest<1>, dig_grid, 0, h->P, D);
        HIPCHK(h, hipGetLastError());
        if (mlm_sort_pairs_u64_u32(b + o_sort, sort_bytes, D.packed, (unsigned long long *)(b + o_kb), D.slot_of, (uint32_t *)(b + o_vb), nb, h->stream) != 0) {
            (void)hipStreamSynchronize(h->stream);
            h->err = "mlm_delta_blocks: the sort of the packed keys failed";
            return MLM_ERR_HIP;
        }
    }
    launch(h, k_delta_join, join_grid, 0, D, D.part + (size_t)dig_grid * MLM_DELTA_ROW, ctrl);
    launch(h, k_fuse_sums, 1u, 0, (const unsigned long long *)D.part, dig_grid + join_grid, sums);
    if (nb) {
        const unsigned int g = std::min(chunks_b, kCropGrid);
        launch(h, k_delta_count, g, 0, (const uint32_t *)D.kind, (uint32_t)MLM_DELTA_K_CHANGED, (uint32_t)MLM_DELTA_K_NEW, nb, chunks_b, chunk_b);
        launch(h, k_crop_scan, 1u, 0, chunk_b, chunks_b, ctrl);
        launch(h, k_delta_rank, g, 0, (const uint32_t *)D.kind, (uint32_t)MLM_DELTA_K_CHANGED, (uint32_t)MLM_DELTA_K_NEW, nb, chunks_b, (const unsigned int *)chunk_b, D.elist);
    }
    if (np) {
        const unsigned int g = std::min(chunks_p, kCropGrid);
        launch(h, k_delta_count, g, 0, (const uint32_t *)D.pstate, (uint32_t)MLM_DELTA_P_GONE, (uint32_t)MLM_DELTA_P_GONE, np, chunks_p, chunk_p);
        launch(h, k_crop_scan, 1u, 0, chunk_p, chunks_p, ctrl + 1);
        launch(h, k_delta_rank, g, 0, (const uint32_t *)D.pstate, (uint32_t)MLM_DELTA_P_GONE, (uint32_t)MLM_DELTA_P_GONE, np, chunks_p, (const unsigned int *)chunk_p, D.glist);
    }
    HIPCHK(h, hipGetLastError());
    const unsigned long long *got;
    if ((rc = read_back(h, (const unsigned long long *)sums, MLM_DELTA_ROW + 2, got))) return rc;
    const unsigned int n_emit = (unsigned int)(got[MLM_DELTA_ROW] & 0xFFFFFFFFull), n_gone = (unsigned int)(got[MLM_DELTA_ROW] >> 32);
    const unsigned int bad_range = (unsigned int)(got[MLM_DELTA_ROW + 1] & 0xFFFFFFFFull), bad_order = (unsigned int)(got[MLM_DELTA_ROW + 1] >> 32);
    if (bad_range || bad_order) {
        h->err = std::string("mlm_delta_blocks: ") + mlm_delta_check_text(bad_range ? 7 : 8);
        return MLM_ERR_INVALID;
    }
    const unsigned long long Ssel = got[MLM_DELTA_S_SELECTED], unchanged = got[MLM_DELTA_S_KIND + MLM_DELTA_K_UNCHANGED], changed = got[MLM_DELTA_S_KIND + MLM_DELTA_K_CHANGED],
                             fresh = got[MLM_DELTA_S_KIND + MLM_DELTA_K_NEW], inbox = got[MLM_DELTA_S_INBOX], gone = got[MLM_DELTA_S_GONE];
    if (Ssel > nb || Ssel != unchanged + changed + fresh || inbox != unchanged + changed + gone || n_emit != changed + fresh || n_gone != gone || gone > np) {
        h->err = "mlm_delta_blocks: the counts of the join are inconsistent";
        return MLM_ERR_HIP;
    }
    const unsigned int Sn = (unsigned int)Ssel, E = n_emit, G = n_gone;
    sum[1] = Sn, sum[3] = (int64_t)inbox, sum[4] = (int64_t)unchanged, sum[5] = (int64_t)changed, sum[6] = (int64_t)fresh, sum[7] = G;
    sum[11] = (int64_t)got[MLM_DELTA_S_EMPTY];
    const bool table_out = cur_keys || cur_digest, block_out = keys || log_odds || occ || infl || kind;
    const char *short_of = table_out && (unsigned int)cap_table < Sn ? "table rows" : block_out && (unsigned int)cap < E ? "emitted blocks" : gone_keys && (unsigned int)cap_gone < G ? "gone keys" : nullptr;
    if (short_of) {
        const bool t = short_of[0] == 't', e = short_of[0] == 'e';
        h->err = std::string("mlm_delta_blocks: ") + std::to_string(t ? Sn : e ? E : G) + " " + short_of + " would be written, the outputs hold " +
                 std::to_string(t ? cap_table : e ? cap : cap_gone);
        report();
        return MLM_ERR_CAPACITY;
    }
    if (flags & MLM_DELTA_DRY) {
        report();
        return MLM_OK;
    }
    // every allocation before the first write: the staging of host outputs — the three sets share one buffer, used one after the other
    // in stream order
    ReadoutChannels<3> rows_ch(h->d_win_stage, {{cur_keys, 3 * sizeof(int32_t)}, {cur_digest, 2 * sizeof(uint64_t)}, {gone_keys, 3 * sizeof(int32_t)}});
    ReadoutChannels<5> ch(h->d_win_stage, {{keys, 3 * sizeof(int32_t)}, {log_odds, C * sizeof(float)}, {occ, C}, {infl, C}, {kind, 1}});
    const size_t page = block_out && E ? page_rows(ch, E) : 0;
    const size_t row_counts[3] = {Sn, Sn, G};
    if ((rc = rows_ch.reserve(h, "mlm_delta_blocks", row_counts)) || (page && (rc = ch.reserve(h, "mlm_delta_blocks", page)))) {
        report();
        return rc;
    }
    const unsigned int Gw = gone_keys ? G : 0u, Sw = table_out ? Sn : 0u;
    if (Sw || Gw) {
        launch(h, k_delta_rows, lanes_grid((size_t)Sn + Gw, kCropGrid), 0, D, table_out ? Sn : 0u, Gw, (int32_t *)rows_ch.at(0, 0), (unsigned long long *)rows_ch.at(1, 0),
               (int32_t *)rows_ch.at(2, 0));
        HIPCHK(h, hipGetLastError());
        if ((rc = rows_ch.copy_out(h, 0, 2, 0, Sw))) return rc;
        if ((rc = rows_ch.copy_out(h, 2, 3, 0, Gw))) return rc;
        sum[9] = Sw, sum[10] = Gw;
    }
    if (page) {
        rc = page_rounds(h, ch, E, page, [&](size_t r0, size_t r1) {
            float *d_lo = (float *)ch.at(1, r0);
            uint8_t *d_occ = (uint8_t *)ch.at(2, r0), *d_infl = (uint8_t *)ch.at(3, r0);
            const int pfw = crop_width(fw, d_lo), pbw = std::min(crop_width(bw, d_occ), crop_width(bw, d_infl));
            MLM_CROP_LAUNCH(k_delta_emit, pfw, pbw, wave_grid(r1 - r0, kCropGrid), h->P, D, (unsigned int)r0, (unsigned int)r1, (int32_t *)ch.at(0, r0), d_lo, d_occ, d_infl,
                            (uint8_t *)ch.at(4, r0));
        });
        if (rc) return rc;
        sum[8] = E;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    report();
    return MLM_OK;
}
} // namespace

int mlm_delta_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int n_prev, const int32_t *prev_keys, const uint64_t *prev_digest, int flags,
                     int cap_table, int32_t *cur_keys, uint64_t *cur_digest, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, uint8_t *kind,
                     int cap_gone, int32_t *gone_keys, int64_t summary[MLM_DELTA_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    MlmAgeSel S{};
    if (const int bad = mlm_delta_check(key_lo, key_dims, n_prev, prev_keys, prev_digest, flags, cap_table, cap, cap_gone, S)) {
        h->err = std::string("mlm_delta_blocks: ") + mlm_delta_check_text(bad);
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    if (rc) return rc;
    return delta_run(h, S, n_prev, prev_keys, prev_digest, flags, cap_table, cur_keys, cur_digest, cap, keys, log_odds, occ, infl, kind, cap_gone, gone_keys, summary);
}
