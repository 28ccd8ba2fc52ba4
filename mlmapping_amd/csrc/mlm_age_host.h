// mlm_age_host.h — host part of mlmap_hip.hip (included behind mlm_fuse_host.h): the driver of mlm_age_blocks.  The rule is
// mlm_age.h's, the kernels are mlm_kernels_age.h's, the compaction is mlm_crop_blocks' (crop_compact).
//
// Order of a call: the handle's scratch and the staging of a host per_block reserved; then — behind every check and every allocation —
// the rule applied, the partial sums added and, with MLM_AGE_DROP, the empty selected blocks counted, scanned and listed; the host reads
// the twelve sums with {D, H} once (the one synchronisation of a call that drops nothing); then the compaction.
#pragma once

namespace {
static_assert(MLM_AGE_SCALE == MLM_AGE_M_SCALE && MLM_AGE_STEP == MLM_AGE_M_STEP && MLM_AGE_OUTSIDE == MLM_AGE_F_OUTSIDE && MLM_AGE_DRY == MLM_AGE_F_DRY &&
                  MLM_AGE_FORGET == MLM_AGE_F_FORGET && MLM_AGE_DROP == MLM_AGE_F_DROP && MLM_AGE_CLEAR_INFL == MLM_AGE_F_CLEAR_INFL &&
                  MLM_AGE_ROW == MLM_AGE_SUMS && MLM_AGE_COLS == MLM_AGE_PB,
              "mlm_age.h restates the constants of include/mlmap_hip.h");

constexpr unsigned int kAgeApplyGrid = 2048; // most workgroups of k_age_apply: a wave takes several blocks, a workgroup writes one row of sums

// everything of mlm_age_blocks behind the argument check and the drain
int age_run(mlm_handle *h, const MlmAgeSel &S, int mode, float amount, float forget, int flags, int32_t *per_block, int64_t *summary) {
    int64_t sum[MLM_AGE_ROW] = {};
    auto report = [&]() {
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    const bool dry = (flags & MLM_AGE_DRY) != 0, drop = (flags & MLM_AGE_DROP) != 0;
    int rc = read_global(h);
    if (rc) return rc;
    const unsigned int nb = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks);
    h->stats.n_blocks = nb; // (as mlm_crop_blocks: mlm_frame_stats follows the calls that may change the block count between frames)
    h->stats.block_capacity = h->P.max_blocks;
    if (nb == 0) {
        report();
        return MLM_OK;
    }
    // the handle's scratch: block states | list | chunk counts | the twelve sums with the control words {D, H} behind them | partial sums
    const unsigned int chunks = (nb + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
    const unsigned int apply_grid = wave_grid(nb, kAgeApplyGrid);
    const size_t w4 = mlm_align256((size_t)nb * 4);
    const size_t o_list = w4, o_ch = 2 * w4, o_ctrl = o_ch + mlm_align256((size_t)chunks * 4), o_part = o_ctrl + 256,
                 total = o_part + mlm_align256((size_t)apply_grid * MLM_AGE_ROW * 8);
    if ((rc = readout_reserve(h, h->d_age, total, "mlm_age_blocks"))) return rc;
    // a host per_block goes through the read-outs' staging
    ReadoutChannels<1> ch(h->d_win_stage, {{per_block, MLM_AGE_COLS * sizeof(int32_t)}});
    if ((rc = ch.reserve(h, "mlm_age_blocks", (size_t)nb))) return rc;

    char *b = (char *)h->d_age.p;
    MlmAge G{};
    G.A.R = MlmFuseRule{h->P.lo_min, h->P.lo_max, h->P.lo_sh, 0, 0};
    G.A.mode = mode, G.A.flags = flags, G.A.amount = amount, G.A.forget = forget;
    G.S = S;
    G.nb = nb;
    G.state = (uint32_t *)b;
    G.per_block = (int32_t *)ch.at(0, 0);
    G.part = (unsigned long long *)(b + o_part);
    unsigned int *list = (unsigned int *)(b + o_list), *chunk_cnt = (unsigned int *)(b + o_ch);
    unsigned long long *sums = (unsigned long long *)(b + o_ctrl);
    unsigned int *ctrl = (unsigned int *)(sums + MLM_AGE_ROW); // {D, H}: the thirteenth word of the read-back
    // four voxels per lane where a block's rows are aligned and fill a quarter of a wave at least, else one
    const int V = mlm_crop_float_width(h->P.cells) == 16 && mlm_crop_byte_width(h->P.cells) >= 4 && h->P.cells >= 64 ? 4 : 1;

    HIPCHK(h, hipMemsetAsync(sums, 0, 256, h->stream));
    // From here on the map changes (not with MLM_AGE_DRY).
    if (!dry) mirror_mark_all(h);
    MLM_FUSE_LAUNCH(k_age_apply, V, dry, apply_grid, h->P, G);
    launch(h, k_fuse_sums, 1u, 0, (const unsigned long long *)G.part, apply_grid, sums);
    if (drop && !dry) {
        const unsigned int scan_grid = std::min(chunks, kCropGrid);
        launch(h, k_age_count, scan_grid, 0, (const uint32_t *)G.state, nb, chunks, chunk_cnt);
        launch(h, k_crop_scan, 1u, 0, chunk_cnt, chunks, ctrl);
        launch(h, k_age_list, scan_grid, 0, (const uint32_t *)G.state, nb, chunks, (const unsigned int *)chunk_cnt, ctrl, list);
    }
    HIPCHK(h, hipGetLastError());
    if ((rc = ch.copy_out(h, 0, 1, 0, (size_t)nb))) return rc;
    const unsigned long long *got;
    if ((rc = read_back(h, (const unsigned long long *)sums, MLM_AGE_ROW + 1, got))) return rc;
    for (int k = 4; k < MLM_AGE_ROW; ++k) sum[k] = (int64_t)got[k];
    const unsigned int n_empty = (unsigned int)got[0];
    sum[0] = nb, sum[1] = (int64_t)got[1];
    sum[2] = drop ? n_empty : 0, sum[3] = (int64_t)nb - sum[2];
    if (drop && !dry) {
        const unsigned int D = (unsigned int)(got[MLM_AGE_ROW] & 0xFFFFFFFFull), H = (unsigned int)(got[MLM_AGE_ROW] >> 32);
        if (D != n_empty || D > nb || H > std::min(D, nb - D)) {
            h->err = "mlm_age_blocks: the scan of the empty blocks is inconsistent";
            return MLM_ERR_HIP;
        }
        if (D) {
            MlmGlobal g{};
            if ((rc = crop_compact(h, (const unsigned int *)list, nb, D, nb - D, H, g))) return rc;
        }
    }
    report();
    return MLM_OK;
}
} // namespace

int mlm_age_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int mode, float amount, float forget, int flags,
                   int32_t *per_block, int64_t summary[MLM_AGE_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    MlmAgeSel S{};
    if (const int bad = mlm_age_check(key_lo, key_dims, mode, amount, forget, flags, S)) {
        h->err = std::string("mlm_age_blocks: ") + mlm_age_check_text(bad);
        return MLM_ERR_INVALID;
    }
    if (h->P.explore) {
        h->err = "mlm_age_blocks: refused on a frontier-mode handle (frontier, released and observed flags have no aged meaning)";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    if (rc) return rc;
    return age_run(h, S, mode, amount, forget, flags, per_block, summary);
}
