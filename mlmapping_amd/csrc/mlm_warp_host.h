// mlm_warp_host.h — host part of mlmap_hip.hip (included behind mlm_import_blocks and mlm_crop_blocks, whose code paths
// MLM_WARP_REPLACE is made of): the driver of mlm_warp_blocks.  The rule is mlm_warp.h's, the kernels are mlm_kernels_warp.h's.
//
// Order of a call: candidates into the set, the set's used entries counted (the host reads NC), listed and sorted; the gather counts
// per candidate, the emitted candidates numbered (the host reads E and the four sums); then — behind every check and every
// allocation — the rows written, and with MLM_WARP_REPLACE the dump written once more into the staging of an import, every block
// dropped by crop_run and the staging imported by import_staged.
#pragma once

namespace {
static_assert(MLM_WARP_SEEN == MLM_WARP_F_SEEN && MLM_WARP_REPLACE == MLM_WARP_F_REPLACE && MLM_WARP_DRY == MLM_WARP_F_DRY,
              "mlm_warp.h restates the flags of include/mlmap_hip.h");
static_assert(MLM_WARP_ROW == 4 + MLM_WARP_SUMS, "summary: four block counts, then the sums of k_warp_sums");

// everything of mlm_warp_blocks behind the argument check and the drain
int warp_run(mlm_handle *h, const MlmWarpPlan &W, int flags, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, int64_t *summary) {
    int64_t sum[MLM_WARP_ROW] = {};
    auto report = [&]() {
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    int rc = read_global(h);
    if (rc) return rc;
    const unsigned int nb = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks);
    sum[0] = nb;
    const bool any_out = keys || log_odds || occ || infl, replace = (flags & MLM_WARP_REPLACE) && !(flags & MLM_WARP_DRY);
    const MlmWarpGeom G{h->P.d_sub, h->P.d_glb, h->P.d_sub_half, h->P.n};
    const size_t C = (size_t)h->P.cells;
    MlmWarp Q{};
    Q.W = W;
    Q.cell_m = C <= mlm_host::STRIP_MAGIC_MAX_I ? mlm_host::strip_magic((unsigned int)h->P.n) : 0u;
    unsigned int NC = 0, E = 0, set_chunks = 0, *set_cnt = nullptr;
    unsigned long long nt = 0; // entries of the candidate set
    if (nb) {
        // the candidate set: at least twice the keys the source blocks can name | its chunk counts | control words
        const unsigned long long most = (unsigned long long)nb * mlm_warp_span(W, G, 0) * mlm_warp_span(W, G, 1) * mlm_warp_span(W, G, 2);
        nt = 1024;
        while (nt < 2 * most) nt <<= 1;
        if (nt > (1ull << 30)) {
            h->err = "mlm_warp_blocks: " + std::to_string(nb) + " source blocks name too many candidate blocks for one call";
            report();
            return MLM_ERR_CAPACITY;
        }
        set_chunks = (unsigned int)((nt + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK);
        const size_t o_cnt = (size_t)nt * 8, o_ctrl = o_cnt + mlm_align256((size_t)set_chunks * 4);
        if ((rc = readout_reserve(h, h->d_warp_set, o_ctrl + 256, "mlm_warp_blocks"))) {
            report();
            return rc;
        }
        unsigned long long *set = (unsigned long long *)h->d_warp_set.p;
        set_cnt = (unsigned int *)((char *)h->d_warp_set.p + o_cnt);
        unsigned int *set_ctrl = (unsigned int *)((char *)h->d_warp_set.p + o_ctrl);
        HIPCHK(h, hipMemsetAsync(set, 0xFF, (size_t)nt * 8, h->stream));
        HIPCHK(h, hipMemsetAsync(set_ctrl, 0, MLM_WARP_CTRL_WORDS * 4, h->stream));
        launch(h, k_warp_candidates, lanes_grid(nb, kCropGrid), 0, h->P, W, nb, set, (uint32_t)(nt - 1), set_ctrl);
        launch(h, k_warp_set_count, std::min(set_chunks, kCropGrid), 0, (const unsigned long long *)set, (unsigned int)nt, set_chunks, set_cnt);
        launch(h, k_crop_scan, 1u, 0, set_cnt, set_chunks, set_ctrl);
        HIPCHK(h, hipGetLastError());
        const unsigned int *c;
        if ((rc = read_back(h, (const unsigned int *)set_ctrl, MLM_WARP_CTRL_WORDS, c))) return rc;
        NC = c[0];
        if (c[1] || NC > most) {
            h->err = "mlm_warp_blocks: the candidate set is inconsistent";
            return MLM_ERR_HIP;
        }
    }
    sum[1] = NC;
    if (NC) {
        // keys (as listed, then sorted) | the sort's values, twice | four counters per candidate | the emitted list | chunk counts |
        // control words and sums | the sort's scratch
        const unsigned int chunks = (NC + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
        const size_t sort_bytes = mlm_sort_temp_bytes(NC);
        const size_t o_kb = mlm_align256((size_t)NC * 8), o_va = 2 * o_kb, o_vb = o_va + mlm_align256((size_t)NC * 4), o_cnt = o_vb + mlm_align256((size_t)NC * 4),
                     o_el = o_cnt + mlm_align256((size_t)NC * 16), o_ch = o_el + mlm_align256((size_t)NC * 4), o_ctrl = o_ch + mlm_align256((size_t)chunks * 4),
                     o_sort = o_ctrl + 256, total = o_sort + mlm_align256(sort_bytes);
        if ((rc = readout_reserve(h, h->d_warp, total, "mlm_warp_blocks"))) {
            report();
            return rc;
        }
        char *b = (char *)h->d_warp.p;
        unsigned long long *keys_a = (unsigned long long *)b, *keys_b = (unsigned long long *)(b + o_kb);
        uint32_t *vals_a = (uint32_t *)(b + o_va), *vals_b = (uint32_t *)(b + o_vb), *cnt = (uint32_t *)(b + o_cnt);
        unsigned int *elist = (unsigned int *)(b + o_el), *chunk_cnt = (unsigned int *)(b + o_ch), *ctrl = (unsigned int *)(b + o_ctrl);
        unsigned long long *sums = (unsigned long long *)(b + o_ctrl + 64);
        launch(h, k_warp_set_list, std::min(set_chunks, kCropGrid), 0, (const unsigned long long *)h->d_warp_set.p, (unsigned int)nt, set_chunks,
               (const unsigned int *)set_cnt, keys_a, vals_a, NC);
        HIPCHK(h, hipGetLastError());
        if (mlm_sort_pairs_u64_u32(b + o_sort, sort_bytes, keys_a, keys_b, vals_a, vals_b, NC, h->stream) != 0) {
            h->err = "mlm_warp_blocks: the sort of the candidate keys failed";
            return MLM_ERR_HIP;
        }
        Q.cand = keys_b, Q.nc = NC, Q.cnt = cnt, Q.elist = elist;
        HIPCHK(h, hipMemsetAsync(ctrl, 0, 256, h->stream));
        launch(h, k_warp_count, wave_grid(NC, kCropGrid), 0, h->P, Q);
        launch(h, k_warp_sums, std::min(grid_for(NC) / 8 + 1, 64u), 0, (const uint32_t *)cnt, NC, sums);
        const unsigned int grid = std::min(chunks, kCropGrid);
        launch(h, k_warp_emit_count, grid, 0, (const uint32_t *)cnt, NC, chunks, chunk_cnt);
        launch(h, k_crop_scan, 1u, 0, chunk_cnt, chunks, ctrl);
        launch(h, k_warp_emit_list, grid, 0, (const uint32_t *)cnt, NC, chunks, (const unsigned int *)chunk_cnt, elist);
        HIPCHK(h, hipGetLastError());
        const unsigned long long *back; // the control words, then (from byte 64 on) the sums
        if ((rc = read_back(h, (const unsigned long long *)ctrl, 12, back))) return rc;
        E = (unsigned int)(back[0] & 0xFFFFFFFFull);
        for (int k = 0; k < MLM_WARP_SUMS; ++k) sum[4 + k] = (int64_t)back[8 + k];
        if (E > NC) {
            h->err = "mlm_warp_blocks: the scan of the emitted flags is inconsistent";
            return MLM_ERR_HIP;
        }
    }
    sum[2] = E;
    if (any_out && (unsigned int)cap < E) {
        h->err = "mlm_warp_blocks: " + std::to_string(E) + " blocks would be emitted, the outputs hold " + std::to_string(cap);
        report();
        return MLM_ERR_CAPACITY;
    }
    if (flags & MLM_WARP_DRY) {
        report();
        return MLM_OK;
    }
    // every allocation before the first write: the staging of host outputs, and for a replacing call the import's staging and a pool
    // that holds the E blocks
    ReadoutChannels<4> ch(h->d_win_stage, {{keys, 3 * sizeof(int32_t)}, {log_odds, C * sizeof(float)}, {occ, C}, {infl, C}});
    const size_t rows = any_out && E ? page_rows(ch, E) : E;
    if (any_out && E && (rc = ch.reserve(h, "mlm_warp_blocks", rows))) {
        report();
        return rc;
    }
    DevTmp stage;
    const ImportStage L = import_stage(E, C);
    if (replace) {
        if (E && hipMalloc(&stage.p, L.total) != hipSuccess) {
            (void)hipGetLastError();
            stage.p = nullptr;
            h->err = "mlm_warp_blocks: no device memory for " + std::to_string(L.total >> 20) + " MB of import staging";
            report();
            return MLM_ERR_CAPACITY;
        }
        if (E > (unsigned int)h->P.max_blocks) { // (what the import behind a crop of everything would do, ahead of the crop)
            const size_t most = (size_t)(0x7FFFFFFFll / h->P.cells);
            rc = !h->pool_grow ? MLM_ERR_CAPACITY : grow_pool(h, std::min(most, 2 * (size_t)E));
            if (!rc && E > (unsigned int)h->P.max_blocks) rc = MLM_ERR_CAPACITY;
            if (rc) {
                if (rc == MLM_ERR_CAPACITY && !h->pool_grow) h->err = "mlm_warp_blocks: the pool cannot hold the " + std::to_string(E) + " emitted blocks (raise mlm_limits.max_blocks)";
                report();
                return rc;
            }
        }
    }
    if (any_out && E) {
        rc = page_rounds(h, ch, E, rows, [&](size_t r0, size_t r1) {
            launch(h, k_warp_write, wave_grid(r1 - r0, kCropGrid), 0, h->P, Q, (unsigned int)r0, (unsigned int)r1, (int32_t *)ch.at(0, r0),
                   (float *)ch.at(1, r0), (uint8_t *)ch.at(2, r0), (uint8_t *)ch.at(3, r0));
        });
        if (rc) return rc;
        sum[3] = E;
    }
    if (replace) {
        char *d = (char *)stage.p;
        if (E) {
            launch(h, k_warp_write, wave_grid(E, kCropGrid), 0, h->P, Q, 0u, E, (int32_t *)(d + L.o_keys), (float *)(d + L.o_lo), (uint8_t *)(d + L.o_occ),
                   (uint8_t *)(d + L.o_infl));
            HIPCHK(h, hipGetLastError());
        }
        // drop every block (the mirror forgets what it knows there), then import the dump
        MlmCropBox all{};
        for (int a = 0; a < 3; ++a) all.lo[a] = INT32_MIN, all.hi[a] = INT32_MAX;
        all.inside = 1;
        if ((rc = crop_run(h, all, MLM_CROP_INSIDE, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
        if (E) {
            mirror_mark_all(h);
            if ((rc = ensure_free_blocks_idle(h, E))) return rc;
            if ((rc = import_staged(h, d, L, (int)E, true, true, true, false))) return rc;
        }
        h->stats.n_blocks = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks);
        h->stats.block_capacity = h->P.max_blocks;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    report();
    return MLM_OK;
}
} // namespace

int mlm_warp_blocks(mlm_handle *h, const double T_sd[12], const int32_t key_lo[3], const int32_t key_dims[3], int flags, int cap, int32_t *keys,
                    float *log_odds, uint8_t *occ, uint8_t *infl, int64_t summary[MLM_WARP_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    MlmWarpPlan W{};
    if (const int bad = mlm_warp_check(T_sd, key_lo, key_dims, flags, cap, W)) {
        h->err = std::string("mlm_warp_blocks: ") + mlm_warp_check_text(bad);
        return MLM_ERR_INVALID;
    }
    if ((flags & MLM_WARP_REPLACE) && h->P.explore) {
        h->err = "mlm_warp_blocks: MLM_WARP_REPLACE on a frontier-mode handle (frontier and released flags have no resampled meaning)";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc) return rc;
    return warp_run(h, W, flags, cap, keys, log_odds, occ, infl, summary);
}
