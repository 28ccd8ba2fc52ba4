// mlm_fuse_host.h — host part of mlmap_hip.hip (included behind mlm_warp_host.h): the driver of mlm_fuse_blocks.  The rule is
// mlm_fuse.h's, the kernels are mlm_kernels_fuse.h's.
//
// Order of a call: the handle's scratch, the staging of host sources and of a host per_row reserved; the sources copied; the probe,
// the sort of the packed keys and the neighbour compare, the created rows ranked (the host reads {created, range flag, duplicate
// flag}: the first synchronisation); the pool grown if the created blocks need it; then — behind every check and every allocation —
// the created blocks entered, the block count set and the rule applied (the second synchronisation).
#pragma once

namespace {
static_assert(MLM_FUSE_ADD == MLM_FUSE_M_ADD && MLM_FUSE_MAX == MLM_FUSE_M_MAX && MLM_FUSE_TAKE == MLM_FUSE_M_TAKE && MLM_FUSE_FILL == MLM_FUSE_M_FILL &&
                  MLM_FUSE_DRY == MLM_FUSE_F_DRY && MLM_FUSE_ROW == MLM_FUSE_SUMS && MLM_FUSE_COLS == MLM_FUSE_PR,
              "mlm_fuse.h restates the constants of include/mlmap_hip.h");

constexpr unsigned int kFuseApplyGrid = 1024; // most workgroups of k_fuse_apply: a wave takes several rows, a workgroup writes one row of sums

#define MLM_FUSE_LAUNCH(K, v, dry, grid, ...)                                                                            \
    do {                                                                                                                 \
        if ((v) == 4 && (dry)) hipLaunchKernelGGL((K<4, true>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__); \
        else if ((v) == 4) hipLaunchKernelGGL((K<4, false>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);    \
        else if (dry) hipLaunchKernelGGL((K<1, true>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);          \
        else hipLaunchKernelGGL((K<1, false>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);                  \
    } while (0)

// everything of mlm_fuse_blocks behind the argument check and the drain (n > 0)
int fuse_run(mlm_handle *h, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl, int mode, int flags,
             int32_t *per_row, int64_t *summary) {
    int64_t sum[MLM_FUSE_ROW] = {};
    auto report = [&]() {
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    const bool dry = (flags & MLM_FUSE_DRY) != 0;
    int rc = read_global(h);
    if (rc) return rc;
    const unsigned int nb = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks), N = (unsigned int)n;
    const size_t C = (size_t)h->P.cells;

    // the handle's scratch: row slots | row flags | created slots | packed keys, twice | the sort's values, twice | chunk counts |
    // control words and sums | the apply's partial sums | the sort's scratch
    const unsigned int chunks = (N + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
    const size_t sort_bytes = mlm_sort_temp_bytes(N);
    const size_t w4 = mlm_align256((size_t)N * 4), w8 = mlm_align256((size_t)N * 8);
    const size_t o_flag = w4, o_new = 2 * w4, o_ka = 3 * w4, o_kb = o_ka + w8, o_va = o_kb + w8, o_vb = o_va + w4, o_ch = o_vb + w4,
                 o_ctrl = o_ch + mlm_align256((size_t)chunks * 4), o_part = o_ctrl + 256,
                 o_sort = o_part + mlm_align256((size_t)kFuseApplyGrid * MLM_FUSE_ROW * 8), total = o_sort + mlm_align256(sort_bytes);
    if ((rc = readout_reserve(h, h->d_fuse, total, "mlm_fuse_blocks"))) return rc;
    // a host per_row goes through the read-outs' staging
    ReadoutChannels<1> ch(h->d_win_stage, {{per_row, MLM_FUSE_COLS * sizeof(int32_t)}});
    if ((rc = ch.reserve(h, "mlm_fuse_blocks", (size_t)N))) return rc;
    // host sources staged whole in one allocation; device sources are read in place
    const void *src[4] = {keys, log_odds, occ, infl};
    const size_t bytes[4] = {(size_t)N * 12, (size_t)N * C * 4, (size_t)N * C, (size_t)N * C};
    size_t off[4] = {}, stage_bytes = 0;
    bool staged[4] = {};
    for (int k = 0; k < 4; ++k) {
        staged[k] = src[k] && !readout_in_place(src[k]);
        off[k] = stage_bytes;
        if (staged[k]) stage_bytes += mlm_align256(bytes[k]);
    }
    DevTmp stage;
    if (stage_bytes && hipMalloc(&stage.p, stage_bytes) != hipSuccess) {
        (void)hipGetLastError();
        stage.p = nullptr;
        h->err = "mlm_fuse_blocks: no device memory for " + std::to_string(stage_bytes >> 20) + " MB of staging";
        return MLM_ERR_CAPACITY;
    }
    for (int k = 0; k < 4; ++k)
        if (staged[k]) {
            const hipError_t e = hipMemcpyAsync((char *)stage.p + off[k], src[k], bytes[k], hipMemcpyDefault, h->stream);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(h->stream);
                h->err = std::string("mlm_fuse_blocks: ") + hipGetErrorString(e);
                return MLM_ERR_HIP;
            }
            src[k] = (char *)stage.p + off[k];
        }

    char *b = (char *)h->d_fuse.p;
    MlmFuse F{};
    F.R = MlmFuseRule{h->P.lo_min, h->P.lo_max, h->P.lo_sh, mode, infl ? 1 : 0};
    F.n = N, F.nb = nb;
    F.keys = (const int32_t *)src[0], F.lo = (const float *)src[1], F.occ = (const uint8_t *)src[2], F.infl = (const uint8_t *)src[3];
    F.row_slot = (int32_t *)b, F.row_flag = (uint32_t *)(b + o_flag), F.row_new = (int32_t *)(b + o_new);
    F.per_row = (int32_t *)ch.at(0, 0);
    unsigned long long *keys_a = (unsigned long long *)(b + o_ka), *keys_b = (unsigned long long *)(b + o_kb);
    uint32_t *vals_a = (uint32_t *)(b + o_va), *vals_b = (uint32_t *)(b + o_vb);
    unsigned int *chunk_cnt = (unsigned int *)(b + o_ch), *ctrl = (unsigned int *)(b + o_ctrl);
    unsigned long long *sums = (unsigned long long *)(b + o_ctrl + 64);
    F.part = (unsigned long long *)(b + o_part);
    // the widest lane path the rows' length and the sources' alignment allow: four voxels (16 bytes of log-odds, a dword of classes) or one
    const int fw = mlm_crop_float_width(h->P.cells), bw = mlm_crop_byte_width(h->P.cells);
    const int V = crop_width(fw, F.lo) == 16 && bw >= 4 && crop_width(4, F.occ) == 4 && crop_width(4, F.infl) == 4 ? 4 : 1;

    HIPCHK(h, hipMemsetAsync(ctrl, 0, 256, h->stream));
    const unsigned int rows_grid = wave_grid(N, kCropGrid), scan_grid = std::min(chunks, kCropGrid);
    launch(h, V == 4 ? k_fuse_probe<4> : k_fuse_probe<1>, rows_grid, 0, h->P, F, keys_a, vals_a, ctrl);
    HIPCHK(h, hipGetLastError());
    if (N > 1) {
        if (mlm_sort_pairs_u64_u32(b + o_sort, sort_bytes, keys_a, keys_b, vals_a, vals_b, N, h->stream) != 0) {
            (void)hipStreamSynchronize(h->stream);
            h->err = "mlm_fuse_blocks: the sort of the packed keys failed";
            return MLM_ERR_HIP;
        }
        launch(h, k_fuse_dups, lanes_grid(N, kCropGrid), 0, (const unsigned long long *)keys_b, N, ctrl);
    }
    launch(h, k_fuse_count, scan_grid, 0, F, chunks, chunk_cnt);
    launch(h, k_crop_scan, 1u, 0, chunk_cnt, chunks, ctrl);
    launch(h, k_fuse_rank, scan_grid, 0, F, chunks, (const unsigned int *)chunk_cnt);
    HIPCHK(h, hipGetLastError());
    const unsigned int *c;
    if ((rc = read_back(h, (const unsigned int *)ctrl, MLM_FUSE_CTRL_WORDS, c))) return rc;
    if (c[1] || c[2]) {
        h->err = std::string("mlm_fuse_blocks: ") + mlm_fuse_check_text(c[1] ? 5 : 6);
        report();
        return MLM_ERR_INVALID;
    }
    const unsigned int created = c[0];
    if (created > N) {
        h->err = "mlm_fuse_blocks: the scan of the created rows is inconsistent";
        return MLM_ERR_HIP;
    }
    if (!dry && created) {
        // the pool must hold the created blocks before anything is written
        if ((size_t)nb + created > (size_t)h->P.max_blocks) {
            rc = h->pool_grow ? ensure_free_blocks_idle(h, created) : MLM_OK; // (grow_pool says why it could not)
            if (!rc && (size_t)nb + created > (size_t)h->P.max_blocks) {
                h->err = "mlm_fuse_blocks: the pool cannot hold the " + std::to_string(created) + " created blocks (raise mlm_limits.max_blocks)";
                rc = MLM_ERR_CAPACITY;
            }
            if (rc) {
                report();
                return rc;
            }
        }
        // From here on the map changes.
        mirror_mark_all(h);
        launch(h, k_fuse_create, lanes_grid(N, kCropGrid), 0, h->P, F, created);
        HIPCHK(h, hipGetLastError());
        h->h_g->n_blocks = nb + created; // (k_fuse_create sets the device's)
        for (int k = 0; k < MLM_SETS; ++k) h->h_gb[k]->n_blocks = nb + created;
    } else if (!dry) {
        mirror_mark_all(h);
    }
    const unsigned int apply_grid = wave_grid(N, kFuseApplyGrid);
    MLM_FUSE_LAUNCH(k_fuse_apply, V, dry, apply_grid, h->P, F);
    launch(h, k_fuse_sums, 1u, 0, (const unsigned long long *)F.part, apply_grid, sums);
    HIPCHK(h, hipGetLastError());
    if ((rc = ch.copy_out(h, 0, 1, 0, (size_t)N))) return rc;
    if ((rc = read_back(h, sums, MLM_FUSE_ROW, sum))) return rc;
    sum[0] = N, sum[2] = created;
    if (!dry) {
        h->stats.n_blocks = nb + created;
        h->stats.block_capacity = h->P.max_blocks;
    }
    report();
    return MLM_OK;
}
} // namespace

int mlm_fuse_blocks(mlm_handle *h, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl, int mode, int flags,
                    int32_t *per_row, int64_t summary[MLM_FUSE_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (const int bad = mlm_fuse_check(n, keys, log_odds, occ, mode, flags)) {
        h->err = std::string("mlm_fuse_blocks: ") + mlm_fuse_check_text(bad);
        return MLM_ERR_INVALID;
    }
    if (!(flags & MLM_FUSE_DRY) && h->P.explore) {
        h->err = "mlm_fuse_blocks: on a frontier-mode handle only MLM_FUSE_DRY (frontier and released flags have no fused meaning)";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    if (rc) return rc;
    if (n == 0) {
        if (summary) std::memset(summary, 0, MLM_FUSE_ROW * sizeof(int64_t));
        return MLM_OK;
    }
    return fuse_run(h, n, keys, log_odds, occ, infl, mode, flags, per_row, summary);
}
