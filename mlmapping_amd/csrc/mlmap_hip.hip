// mlmap_hip.hip — host side of libmlmap_hip.so: the C ABI of include/mlmap_hip.h.
//
// Host work per frame is O(1): the pose composition T_ls (map_awareness.cpp:184-186, mlm_host.h), the bookkeeping of
// the emulated libstdc++ rehash policy of hit_idx_odds_hashmap, and kernel launches.  All per-point / per-cell /
// per-voxel work runs in the kernels of mlm_kernels_sector.h (default path) and mlm_kernels.h / mlm_kernels_explore.h.  There is no
// CPU fallback: every entry point fails with MLM_ERR_HIP when the device is unavailable.
//
// ONE device translation unit (the kernels live in headers and are launched from here); the host driver is cut into parts that
// are included in this order: mlm_plan.h (host only: what mlm_create decides without the device) -> mlm_handle.h (the handle, knobs, launch helpers) -> mlm_stage_a.h (Stage A launches, exact
// ordering, statistics) -> mlm_explore_host.h (frontier mode) -> mlm_submit.h (submission, drain / replay, single-frame graph)
// -> mlm_resources.h (device memory: mlm_create's stages, pool growth, frame slots, queries' launcher) -> mlm_mirror.h (host mirror of the map for small
// query batches) -> mlm_readout.h (what the read-outs share: box check, kept buffers, pinned control block, staging of host arrays
// and the loops over it, ESDF tiles, settle loop); this file
// holds the extern "C" entry points.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>
#include <atomic>
#include <chrono>

#include "../../include/mlmap_hip.h"
#include "mlm_kernels_explore.h"
#include "mlm_kernels_sector.h"
#include "mlm_kernels_window.h"
#include "mlm_kernels_esdf.h"
#include "mlm_kernels_grid.h"
#include "mlm_kernels_rays.h"
#include "mlm_kernels_render.h"
#include "mlm_kernels_boxes.h"
#include "mlm_kernels_nearest.h"
#include "mlm_kernels_sweeps.h"
#include "mlm_kernels_views.h"
#include "mlm_kernels_reach.h"
#include "mlm_kernels_route.h"
#include "mlm_kernels_path.h"
#include "mlm_kernels_score.h"
#include "mlm_kernels_clearance.h"
#include "mlm_kernels_cluster.h"
#include "mlm_kernels_mesh.h"
#include "mlm_kernels_octree.h"
#include "mlm_kernels_crop.h"
#include "mlm_kernels_warp.h"
#include "mlm_kernels_fuse.h"
#include "mlm_kernels_age.h"
#include "mlm_kernels_delta.h"
#include "mlm_kernels_pack.h"
#include "mlm_host.h"
#include "mlm_plan.h"
#include "mlm_mapview.h"

#include "mlm_handle.h"
#include "mlm_stage_a.h"
#include "mlm_explore_host.h"
#include "mlm_submit.h"
#include "mlm_resources.h"
#include "mlm_mirror.h"
#include "mlm_readout.h"

extern "C" {

int mlm_abi_version(void) { return MLM_ABI_VERSION; }

int mlm_debug_set(const char *name, long long value) {
    if (!name) return MLM_ERR_INVALID;
    bool known = false;
    for (const char *k : kKnobNames) known = known || strcmp(k, name) == 0;
    if (!known) return MLM_ERR_INVALID;
    if (!knob_value_ok(name, value)) return MLM_ERR_INVALID;
    KnobStore &k = knob_store();
    std::lock_guard<std::mutex> lock(k.mu);
    k.v[name] = value;
    return MLM_OK;
}
int mlm_debug_reset(void) {
    KnobStore &k = knob_store();
    std::lock_guard<std::mutex> lock(k.mu);
    k.v.clear();
    return MLM_OK;
}

int mlm_debug_probe_seeds(mlm_handle *h, double out4[4]) {
    if (!h || !out4) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long *d = nullptr;
    HIPCHK(h, hipMalloc((void **)&d, 4 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_seeds, dim3(1024), dim3(256), 0, h->stream, d, 1u << 26);
        e = hipMemcpyAsync(out4, d, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d);
    if (e != hipSuccess) {
        h->err = std::string("mlm_debug_probe_seeds: ") + hipGetErrorString(e);
        return MLM_ERR_HIP;
    }
    return MLM_OK;
}

int mlm_debug_clocks(mlm_handle *h, double out_us[8], int reset) {
    if (!h || !out_us) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    for (int i = 0; i < 8; ++i) {
        out_us[i] = h->clk[i];
        if (reset) h->clk[i] = 0.0;
    }
    return MLM_OK;
}

int mlm_host_register(mlm_handle *h, const void *ptr, size_t bytes) {
    if (!h || !ptr || bytes == 0) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterDefault));
    return MLM_OK;
}
int mlm_host_unregister(mlm_handle *h, const void *ptr) {
    if (!h || !ptr) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h); // (nothing may still be reading from it)
    if (rc) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipHostUnregister(const_cast<void *>(ptr)));
    return MLM_OK;
}

const char *mlm_last_error(mlm_handle *h) { return h ? h->err.c_str() : "null handle"; }

// The plan (mlm_plan.h) decides everything that needs no device — and makes every refusal that needs none —, the stages of
// mlm_resources.h then build the handle's device state with it, in this order.
int mlm_create(const mlm_config *cfg, const mlm_limits *lim_in, int device, mlm_handle **out) {
    if (!cfg || !out) return MLM_ERR_INVALID;
    *out = nullptr;
    if (!mlm_plan_args_ok(*cfg)) return MLM_ERR_INVALID;
    mlm_handle *h = new mlm_handle();
    *out = h; // returned even on failure so that mlm_last_error can be read; caller must mlm_destroy it
    h->device = device;
    h->cfg = *cfg;
    int rc, n_cu = 0;
    if ((rc = open_device(h, &n_cu))) return rc;
    const MlmPlan plan = mlm_plan(*cfg, lim_in, knob, n_cu);
    h->lim = plan.lim;
    if (plan.status != MLM_OK) {
        h->err = plan.err;
        return plan.status;
    }
    h->P = plan.P;
    static_cast<MlmHandlePlan &>(*h) = plan.H;
    static_cast<MlmMirrorLimits &>(h->mir) = plan.mir;
    mirror_apply_limit(h);
    const MlmDev &P = h->P;
    if (getenv("MLM_DEBUG_CREATE"))
        fprintf(stderr, "[create] sector path %d: LDS %u bytes per column (table %u entries), frame-local grid %d x %d x %d in %d tiles of edge %d (%u bytes of LDS each)\n",
                (int)h->use_sectors, P.sec_lds_bytes, P.sec_tab, P.lv_nx, P.lv_ny, P.lv_nz, P.n_tiles, 1 << P.tile_sh, h->tile_lds_bytes);
    if ((rc = create_main_stream(h, n_cu))) return rc;
    if ((rc = set_kernel_lds(h))) return rc;
    if ((rc = upload_tables(h, plan))) return rc;
    if ((rc = alloc_map(h))) return rc;
    if ((rc = create_stage_a(h, n_cu))) return rc;
    h->map_bytes = h->alloc_bytes;
    if ((rc = alloc_slots(h, plan.slot))) return rc;
    if ((rc = alloc_ct_shared(h))) return rc;
    if ((rc = upload_slot_tab(h))) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    const size_t NS = h->slots.size();
    if (getenv("MLM_DEBUG_CREATE"))
        fprintf(stderr, "[create] device memory: %.2f GB (%zu frame slots in %d sets of %d, %.3f GB each; the map and the shared tables %.2f GB)\n",
                h->alloc_bytes / 1e9, NS, h->n_sets, h->lim.max_batch, NS ? (h->alloc_bytes - h->map_bytes) / 1e9 / NS : 0.0, h->map_bytes / 1e9);
    return MLM_OK;
}

int mlm_destroy(mlm_handle *h) {
    if (!h) return MLM_ERR_INVALID;
    h->mu.lock(); // waits for a call in flight on another thread; the caller guarantees that none starts after this
    h->mu.unlock();
    if (!h->stream) { // creation failed before the device was touched
        delete h;
        return MLM_OK;
    }
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    for (void *p : h->allocs)
        if (p) hipFree(p);
    for (auto &S : h->slots) {
        if (S.d_img) hipFree(S.d_img);
        if (S.d_pix) hipFree(S.d_pix);
        if (S.d_pts) hipFree(S.d_pts);
    }
    if (h->h_ctr_all) hipHostFree(h->h_ctr_all);
    if (h->h_frame_tab) hipHostFree(h->h_frame_tab);
    for (int k = 0; k < MLM_SETS; ++k) {
        if (h->stage_a_done[k]) hipEventDestroy(h->stage_a_done[k]);
        if (h->ex_counts[k]) hipEventDestroy(h->ex_counts[k]);
        if (h->ex_bc_done[k]) hipEventDestroy(h->ex_bc_done[k]);
        if (h->set_free[k]) hipEventDestroy(h->set_free[k]);
    }
    for (int k = 0; k < MLM_SETS; ++k)
        if (h->stream_as[k]) hipStreamDestroy(h->stream_as[k]);

    for (auto &g : h->graphs) hipGraphExecDestroy(g.exec);
    if (h->h_stage) hipHostFree(h->h_stage);
    if (h->h_ctrl) hipHostFree(h->h_ctrl);
    if (h->upload_ev) hipEventDestroy(h->upload_ev);
    if (h->host_read_ev) hipEventDestroy(h->host_read_ev);
    if (h->inputs_ready) hipEventDestroy(h->inputs_ready);
    if (h->fb_done) hipEventDestroy(h->fb_done);
    if (h->d_f32) hipFree(h->d_f32);
    for (int k = 0; k < MLM_SETS; ++k)
        if (h->d_img_set[k]) hipFree(h->d_img_set[k]);
    if (h->d_qpos) hipFree(h->d_qpos);
    if (h->d_qout) hipFree(h->d_qout);
    mirror_free(h);
    if (h->mir.eager_ev) hipEventDestroy(h->mir.eager_ev);
    if (h->mir.stat) hipHostFree(h->mir.stat);
    if (h->h_g) hipHostFree(h->h_g);
    for (int k = 0; k < MLM_SETS; ++k) {
        if (h->batch_done[k]) hipEventDestroy(h->batch_done[k]);
        if (h->h_gb[k]) hipHostFree(h->h_gb[k]);
    }
    for (auto &k : h->kpool) {
        hipEventDestroy(k.a);
        hipEventDestroy(k.b);
    }
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;
    return MLM_OK;
}

int mlm_set_stream(mlm_handle *h, void *s) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)s;
    h->own_stream = false;
    if (!h->inputs_ready) HIPCHK(h, hipEventCreateWithFlags(&h->inputs_ready, hipEventDisableTiming));
    return MLM_OK;
}

int mlm_integrate_depth_batch_dev(mlm_handle *h, const uint16_t *img_dev, int n_frames, size_t frame_stride, int width,
                                  int height, int row_stride, const double *q_wb, const double *t_wb) {
    if (!h || !img_dev || n_frames < 0 || !q_wb || !t_wb || width <= 0 || height <= 0 || row_stride < width)
        return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if ((long long)width * height > h->lim.max_points) {
        h->err = "frame has more points than mlm_limits.max_points";
        return MLM_ERR_CAPACITY;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int K = h->lim.max_batch;
    for (int k0 = 0; k0 < n_frames; k0 += K) {
        const int n = std::min(K, n_frames - k0);
        for (int j = 0; j < n; ++j) {
            MlmSlot &S = cur_slot(h, j);
            S.F = MlmFrame{};
            frame_setup(h, q_wb + 4 * (size_t)(k0 + j), t_wb + 3 * (size_t)(k0 + j), S.F);
            S.F.img = img_dev + (size_t)(k0 + j) * frame_stride;
            frame_image(S.F, width, height, row_stride);
            S.F.n = width * height;
            S.mode = 0;
        }
        const int rc = run_slots(h, n);
        if (rc) return rc;
    }
    return MLM_OK;
}

int mlm_integrate_depth_batch(mlm_handle *h, const uint16_t *img_host, int n_frames, size_t frame_stride, int width,
                              int height, int row_stride, const double *q_wb, const double *t_wb) {
    if (!h || !img_host || n_frames < 0 || !q_wb || !t_wb || width <= 0 || height <= 0 || row_stride < width)
        return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if ((long long)width * height > h->lim.max_points) {
        h->err = "frame has more points than mlm_limits.max_points";
        return MLM_ERR_CAPACITY;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int K = h->lim.max_batch;
    const size_t n_px = (size_t)row_stride * height;
    const size_t span = mlm_image_span(width, height, row_stride); // (what is read of one frame: the last row is not padded)
    for (int k0 = 0; k0 < n_frames; k0 += K) {
        const int n = std::min(K, n_frames - k0);
        // frames that lie back to back in host memory go up in ONE copy into the slot set's batch buffer (64 copies of 0.6 MB each
        // reach a third of the link's rate); others frame by frame into the slots' own buffers
        const bool packed = frame_stride == n_px && n > 1;
        const int set = h->cur_set;
        hipStream_t up = h->async_mode ? h->stream_as[set] : h->stream; // (the stream this chunk's Stage A runs on, unless it is one frame: run_slots orders that case)
        if (packed) {
            if (h->img_set_cap[set] < (size_t)K * n_px) {
                if (h->d_img_set[set]) {
                    HIPCHK(h, hipStreamSynchronize(h->stream_as[set])); // (its last user is long done: the set is being refilled)
                    hipFree(h->d_img_set[set]);
                }
                h->d_img_set[set] = nullptr;
                h->img_set_cap[set] = 0;
                HIPCHK(h, hipMalloc((void **)&h->d_img_set[set], (size_t)K * n_px * sizeof(uint16_t)));
                h->img_set_cap[set] = (size_t)K * n_px;
            }
            HIPCHK(h, hipMemcpyAsync(h->d_img_set[set], img_host + (size_t)k0 * frame_stride, mlm_batch_span(n, n_px, width, height, row_stride) * sizeof(uint16_t), hipMemcpyHostToDevice, up));
        }
        for (int j = 0; j < n; ++j) {
            MlmSlot &S = cur_slot(h, j);
            if (!packed) {
                int rc = ensure_img(h, S, n_px);
                if (rc) return rc;
                HIPCHK(h, hipMemcpyAsync(S.d_img, img_host + (size_t)(k0 + j) * frame_stride, span * sizeof(uint16_t), hipMemcpyHostToDevice, up));
            }
            S.F = MlmFrame{};
            frame_setup(h, q_wb + 4 * (size_t)(k0 + j), t_wb + 3 * (size_t)(k0 + j), S.F);
            S.F.img = packed ? h->d_img_set[set] + (size_t)j * n_px : S.d_img;
            frame_image(S.F, width, height, row_stride);
            S.F.n = width * height;
            S.mode = 0;
        }
        int rc = borrowed_mark(h, up); // (asynchronous mode: the caller's frames are read by the copies above only)
        if (rc) return rc;
        // (the frames went up on the slot set's Stage A stream; a chunk of ONE frame in synchronous mode is submitted as the
        // single-frame graph on the MAIN stream: run_slots orders it behind the upload — without this the graph raced the copy,
        // found by tests/test_gpu_random_ops.py)
        h->last_upload = up;
        rc = run_slots(h, n);
        const int rc2 = borrowed_wait(h);
        if (rc || rc2) return rc ? rc : rc2;
    }
    return MLM_OK;
}

static int integrate_u16_dev(mlm_handle *h, const uint16_t *img_dev, int width, int height, int row_stride, const int32_t *pixel_idx_dev,
                             const int32_t *raw_dev, int n_idx, const double q_wb[4], const double t_wb[3]);
int mlm_integrate_depth_u16_dev(mlm_handle *h, const uint16_t *img_dev, int width, int height, int row_stride,
                                const int32_t *pixel_idx_dev, int n_idx, const double q_wb[4], const double t_wb[3]) {
    return integrate_u16_dev(h, img_dev, width, height, row_stride, pixel_idx_dev, nullptr, n_idx, q_wb, t_wb);
}
// raw_dev (with pixel_idx_dev): the listed pixels' depths by list position — the image itself is then never read
static int integrate_u16_dev(mlm_handle *h, const uint16_t *img_dev, int width, int height, int row_stride, const int32_t *pixel_idx_dev,
                             const int32_t *raw_dev, int n_idx, const double q_wb[4], const double t_wb[3]) {
    if (!h || !img_dev || width <= 0 || height <= 0 || row_stride < width || !q_wb || !t_wb) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (pixel_idx_dev && n_idx < 0) return MLM_ERR_INVALID;
    const long long n = pixel_idx_dev ? n_idx : (long long)width * height;
    if (n > h->lim.max_points) {
        h->err = "frame has more points than mlm_limits.max_points";
        return MLM_ERR_CAPACITY;
    }
    HIPCHK(h, hipSetDevice(h->device));
    MlmSlot &S = cur_slot(h, 0);
    S.F = MlmFrame{};
    frame_setup(h, q_wb, t_wb, S.F);
    S.F.img = img_dev;
    S.F.pix = pixel_idx_dev;
    S.F.raw = pixel_idx_dev ? raw_dev : nullptr;
    frame_image(S.F, width, height, row_stride);
    S.F.n = (int)n;
    S.mode = pixel_idx_dev ? 1 : 0;
    return run_slots(h, 1);
}

int mlm_integrate_depth_u16(mlm_handle *h, const uint16_t *img, int width, int height, int row_stride,
                            const int32_t *pixel_idx, int n_idx, const double q_wb[4], const double t_wb[3]) {
    if (!h || !img || width <= 0 || height <= 0 || row_stride < width) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    MlmSlot &S = cur_slot(h, 0);
    const size_t n_px = (size_t)row_stride * height;
    int rc = ensure_img(h, S, n_px);
    if (rc) return rc;
    hipStream_t up = upload_stream(h);
    h->last_upload = up;
    HIPCHK(h, hipMemcpyAsync(S.d_img, img, mlm_image_span(width, height, row_stride) * sizeof(uint16_t), hipMemcpyHostToDevice, up));
    if (pixel_idx) {
        if (n_idx < 0 || n_idx > h->lim.max_points) return MLM_ERR_CAPACITY;
        if ((rc = ensure_pix(h, S))) return rc;
        HIPCHK(h, hipMemcpyAsync(S.d_pix, pixel_idx, (size_t)n_idx * sizeof(int32_t), hipMemcpyHostToDevice, up));
    }
    if ((rc = borrowed_mark(h, up))) return rc;
    rc = mlm_integrate_depth_u16_dev(h, S.d_img, width, height, row_stride, pixel_idx ? S.d_pix : nullptr, n_idx, q_wb, t_wb);
    const int rc2 = borrowed_wait(h);
    return rc ? rc : rc2;
}

int mlm_integrate_callback(mlm_handle *h, const void *depth, int is_f32, int width, int height, double t_img,
                           const double odom_p[3], const double odom_q[4], const double odom_v[3], double t_odom,
                           const double imu_w[3], double t_imu, double latency, int sampled, double T_wb_out[7]) {
    if (!h || !depth || width <= 0 || height <= 0 || !odom_p || !odom_q || !odom_v || !imu_w) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const size_t n_px = (size_t)width * height;
    if ((long long)n_px > h->lim.max_points) {
        h->err = "frame has more points than mlm_limits.max_points";
        return MLM_ERR_CAPACITY;
    }
    HIPCHK(h, hipSetDevice(h->device));
    clk_mark(h, -1);
    // ---- pose latency compensation, mlmap.cpp:470-498 (mlm_host.h)
    double qa[4], ta[3];
    compensate_pose(odom_p, odom_q, odom_v, imu_w, t_img, t_odom, t_imu, latency, qa, ta);
    if (T_wb_out) {
        for (int i = 0; i < 4; ++i) T_wb_out[i] = qa[i];
        for (int i = 0; i < 3; ++i) T_wb_out[4 + i] = ta[i];
    }
    // ---- depth image: upload (and convert 32FC1 -> 16UC1 on the device)
    // (nothing in flight — the synchronous case: no read-back of the map-wide flags and no stream synchronisation just to learn that)
    // (frontier mode, nothing queued: the previous call has synchronised)
    int rc = (h->pending.empty() && !h->wait_ticket && (!h->P.explore || h->ex_q.empty())) ? MLM_OK : drain(h);
    if (rc) return rc;
    MlmSlot &S = cur_slot(h, 0);
    rc = ensure_img(h, S, n_px);
    if (rc) return rc;
    std::vector<int32_t> pix;
    if (sampled && h->cfg.sample_cnt > 0 && 2 * (size_t)h->cfg.sample_cnt <= (size_t)h->lim.max_points) {
        // project_depth, mlmap.cpp:311-349 (glibc rand(), v first, zeros skipped).  Only the sampled pixels are ever read
        // by the kernels, so only they travel: the host converts them (same float arithmetic as k_convert_f32_u16), a tiny
        // kernel drops them into the device image at their pixel positions.
        // The indices and depths are staged in a pinned buffer of the handle that the kernels read across the link.  In asynchronous
        // mode the frame is still in flight when this call returns: the buffer is free again because THIS call drained above before
        // sampling (see mlm_handle::h_stage for the invariant).
        const size_t want = (size_t)h->cfg.sample_cnt;
        if (h->stage_cap < 2 * want) {
            if (h->h_stage) hipHostFree(h->h_stage);
            h->h_stage = nullptr;
            h->stage_cap = 0;
            HIPCHK(h, hipHostMalloc((void **)&h->h_stage, 2 * want * sizeof(int32_t), hipHostMallocDefault));
            h->stage_cap = 2 * want;
        }
        size_t n_s = 0;
        int cnt = 0;
        const int max_iter = 2 * h->cfg.sample_cnt;
        int32_t *st_pix = h->h_stage, *st_raw = h->h_stage + want;
        // (the pixel positions a stretch ahead of their reads: every position drawn is one iteration of the reference's loop, and a
        // stretch is never longer than the iterations the loop is certain to make — rand() is called exactly as often, in the same
        // order; the reads, scattered over the frame, then miss the cache together instead of one after the other)
        size_t ahead[128];
        while (n_s < want && cnt < max_iter) {
            const size_t m = std::min<size_t>(std::min<size_t>(want - n_s, (size_t)(max_iter - cnt)), 128);
            for (size_t i = 0; i < m; ++i) {
                const size_t v = static_cast<size_t>(rand() % height);
                const size_t u = static_cast<size_t>(rand() % width);
                ahead[i] = v * (size_t)width + u;
                __builtin_prefetch(is_f32 ? (const void *)((const float *)depth + ahead[i]) : (const void *)((const uint16_t *)depth + ahead[i]));
            }
            cnt += (int)m;
            for (size_t i = 0; i < m; ++i) {
                const size_t at = ahead[i];
                const int r = is_f32 ? mlm_cv_f32_to_u16(((const float *)depth)[at]) : (int)((const uint16_t *)depth)[at];
                if (r == 0) continue;
                st_pix[n_s] = (int32_t)at;
                st_raw[n_s] = r;
                ++n_s;
            }
        }
        // (the 4 KB do not travel by a copy of their own — a call and a copy kernel, a tenth of the call: the pinned buffer is mapped
        // into the device's address space and k_bin_sectors, the list's only reader, takes the samples from it across the link)
        clk_mark(h, 0);
        rc = integrate_u16_dev(h, S.d_img, width, height, width, h->h_stage, h->h_stage + want, (int)n_s, qa, ta);
        clk_mark(h, 5);
        return rc;
    }
    std::vector<uint16_t> host_u16; // needed only by the sampler when the input is float
    if (is_f32) {
        // the converted frame stays in a buffer owned by the handle (no allocation per call)
        if (h->f32_cap < n_px) {
            if (h->d_f32) hipFree(h->d_f32);
            h->d_f32 = nullptr;
            h->f32_cap = 0;
            HIPCHK(h, hipMalloc((void **)&h->d_f32, n_px * sizeof(float)));
            h->f32_cap = n_px;
        }
        float *d_f = h->d_f32;
        hipError_t e = hipMemcpyAsync(d_f, depth, n_px * sizeof(float), hipMemcpyHostToDevice, h->stream_as[h->cur_set]);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_convert_f32_u16, dim3(grid_for(n_px)), dim3(MLM_BLOCK), 0, h->stream_as[h->cur_set], d_f, S.d_img, n_px);
            if (sampled) {
                host_u16.resize(n_px);
                e = hipMemcpyAsync(host_u16.data(), S.d_img, n_px * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream_as[h->cur_set]);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream_as[h->cur_set]); // `depth` is the caller's
        if (e != hipSuccess) {
            h->err = std::string("mlm_integrate_callback: ") + hipGetErrorString(e);
            return MLM_ERR_HIP;
        }
    } else {
        hipStream_t up = sampled ? h->stream_as[h->cur_set] : upload_stream(h); // (the sampled general path synchronises that stream below)
        HIPCHK(h, hipMemcpyAsync(S.d_img, depth, n_px * sizeof(uint16_t), hipMemcpyHostToDevice, up));
        h->last_upload = up;
        if (!sampled && (rc = borrowed_mark(h, up))) return rc;
    }
    if (sampled) { // (sample count larger than half the point capacity: the general path)
        const uint16_t *img = is_f32 ? host_u16.data() : (const uint16_t *)depth;
        const size_t want = (size_t)h->cfg.sample_cnt;
        int cnt = 0;
        const int max_iter = 2 * h->cfg.sample_cnt;
        while (pix.size() < want && cnt < max_iter) {
            cnt++;
            const size_t v = static_cast<size_t>(rand() % height);
            const size_t u = static_cast<size_t>(rand() % width);
            if (img[v * (size_t)width + u] == 0) continue;
            pix.push_back((int32_t)(v * (size_t)width + u));
        }
        if ((rc = ensure_pix(h, S))) return rc;
        if (!pix.empty())
            HIPCHK(h, hipMemcpyAsync(S.d_pix, pix.data(), pix.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream_as[h->cur_set]));
        HIPCHK(h, hipStreamSynchronize(h->stream_as[h->cur_set])); // pix is a local
    }
    clk_mark(h, 0);
    rc = mlm_integrate_depth_u16_dev(h, S.d_img, width, height, width, sampled ? S.d_pix : nullptr, (int)pix.size(), qa, ta);
    {
        const int rc2 = borrowed_wait(h);
        if (!rc) rc = rc2;
    }
    clk_mark(h, 5);
    return rc;
}

int mlm_integrate_points(mlm_handle *h, const double *xyz, int n, const double q_wb[4], const double t_wb[3]) {
    if (!h || (!xyz && n > 0) || n < 0 || !q_wb || !t_wb) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n > h->lim.max_points) {
        h->err = "frame has more points than mlm_limits.max_points";
        return MLM_ERR_CAPACITY;
    }
    HIPCHK(h, hipSetDevice(h->device));
    MlmSlot &S = cur_slot(h, 0);
    {
        const int rc = ensure_pts(h, S);
        if (rc) return rc;
    }
    if (n > 0) {
        hipStream_t up = upload_stream(h);
        h->last_upload = up;
        HIPCHK(h, hipMemcpyAsync(S.d_pts, xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, up));
        const int rc = borrowed_mark(h, up);
        if (rc) return rc;
    }
    S.F = MlmFrame{};
    frame_setup(h, q_wb, t_wb, S.F);
    S.F.pts = S.d_pts;
    S.F.n = n;
    S.F.width = 1;
    S.mode = 2;
    const int rc = run_slots(h, 1), rc2 = borrowed_wait(h);
    return rc ? rc : rc2;
}

int mlm_query_occupancy(mlm_handle *h, const double *pos, int n, int8_t *out) {
    return run_query(h, 0, pos, n, 0.f, 0, out, 1);
}
int mlm_query_occupancy_inflate(mlm_handle *h, const double *pos, int n, float inflate, int8_t *out) {
    return run_query(h, 1, pos, n, inflate, 0, out, 1);
}
int mlm_query_inflate_occupancy(mlm_handle *h, const double *pos, int n, int8_t *out) {
    return run_query(h, 2, pos, n, 0.f, 0, out, 1);
}
int mlm_query_odds(mlm_handle *h, const double *pos, int n, float *out) {
    return run_query(h, 3, pos, n, 0.f, 0, out, sizeof(float));
}
int mlm_query_odd_grad(mlm_handle *h, const double *pos, int n, int max_iter, double *out3) {
    if (max_iter < 0) return MLM_ERR_INVALID;
    return run_query(h, 4, pos, n, 0.f, max_iter, out3, 3 * sizeof(double));
}

int mlm_set_free_in_bound(mlm_handle *h, const double bmin[3], const double bmax[3]) {
    if (!h || !bmin || !bmax) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    // mlmap.cpp:392-396: `for (double x = min; x <= max; x += d)` — the accumulated coordinates, not i*d
    std::vector<double> ax[3];
    for (int a = 0; a < 3; ++a) {
        for (double v = bmin[a]; v <= bmax[a]; v += h->P.d_sub) {
            ax[a].push_back(v);
            if (ax[a].size() > (1u << 22)) return MLM_ERR_INVALID;
        }
        if (ax[a].empty()) return MLM_OK;
    }
    const size_t total = ax[0].size() * ax[1].size() * ax[2].size();
    const size_t na = ax[0].size() + ax[1].size() + ax[2].size();
    {
        const double wlo[3] = {ax[0].front(), ax[1].front(), ax[2].front()}, whi[3] = {ax[0].back(), ax[1].back(), ax[2].back()};
        mirror_mark_world(h, wlo, whi);
    }
    int rc = drain(h);
    if (rc) return rc;
    rc = ensure_query(h, (na + 2) / 3 + 1);
    if (rc) return rc;
    double *d = h->d_qpos;
    HIPCHK(h, hipMemcpyAsync(d, ax[0].data(), ax[0].size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d + ax[0].size(), ax[1].data(), ax[1].size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d + ax[0].size() + ax[1].size(), ax[2].data(), ax[2].size() * 8, hipMemcpyHostToDevice,
                             h->stream));
    launch(h, k_set_free, grid_for(total), 0, h->P, d, (int)ax[0].size(), d + ax[0].size(), (int)ax[1].size(), d + ax[0].size() + ax[1].size(),
           (int)ax[2].size());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_inflate_map(mlm_handle *h, const double ct_pos[3]) {
    if (!h || !ct_pos) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int R = h->cfg.inflate_n, G = h->cfg.inflate_global_n;
    if (R < 0 || G < 0 || R >= h->P.n || G > 16) {
        h->err = "inflate_n must be < subbox_n and inflate_global_n <= 16";
        return MLM_ERR_UNSUPPORTED;
    }
    int rc = drain(h);
    if (rc) return rc;
    rc = ensure_free_blocks_idle(h, (size_t)(2 * G + 3) * (2 * G + 3) * (2 * G + 3)); // (neighbour blocks are allocated: inflate_atpos)
    if (rc) return rc;
    // get_global_idx(ct_pos) (mlmap.cpp:289, map_local.h:148-152)
    const int cgx = (int)std::floor(ct_pos[0] / h->P.d_glb), cgy = (int)std::floor(ct_pos[1] / h->P.d_glb),
              cgz = (int)std::floor(ct_pos[2] / h->P.d_glb);
    const size_t total = (size_t)(2 * G + 1) * (2 * G + 1) * (2 * G + 1) * (size_t)h->P.cells;
    {
        // (the cube of blocks and the neighbours its dilation may reach; a position whose block index leaves int: anywhere)
        const double c[3] = {std::floor(ct_pos[0] / h->P.d_glb), std::floor(ct_pos[1] / h->P.d_glb), std::floor(ct_pos[2] / h->P.d_glb)};
        if (std::fabs(c[0]) < 1e6 && std::fabs(c[1]) < 1e6 && std::fabs(c[2]) < 1e6) {
            const int lo[3] = {cgx - G - 1, cgy - G - 1, cgz - G - 1}, hi[3] = {cgx + G + 1, cgy + G + 1, cgz + G + 1};
            mirror_mark_box(h, lo, hi);
        } else {
            mirror_mark_all(h);
        }
    }
    launch(h, k_inflate_reset, grid_for(total), 0, h->P, cgx, cgy, cgz, G);
    launch(h, k_inflate_spread, grid_for(total), 0, h->P, cgx, cgy, cgz, G, R, 0.1 /* flate_height, map_local.h:65 */);
    HIPCHK(h, hipGetLastError());
    rc = read_global(h);
    if (rc) return rc;
    if (h->h_g->err) {
        h->err = "block pool or block hash table full (raise mlm_limits.max_blocks)";
        clear_device_error(h);
        return MLM_ERR_CAPACITY;
    }
    return MLM_OK;
}

int mlm_block_count(mlm_handle *h, int *n_out) {
    if (!h || !n_out) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = read_global(h);
    if (rc) return rc;
    *n_out = (int)std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks);
    return MLM_OK;
}

int mlm_export_blocks(mlm_handle *h, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, int *n_out) {
    if (!h || cap < 0) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    int n = 0;
    int rc = mlm_block_count(h, &n);
    if (rc) return rc;
    if (n_out) *n_out = n;
    const size_t m = (size_t)std::min(n, cap);
    const size_t C = (size_t)h->P.cells;
    if (m == 0) return MLM_OK;
    if (keys) HIPCHK(h, hipMemcpyAsync(keys, h->P.block_keys, m * 3 * sizeof(int), hipMemcpyDefault, h->stream));
    if (log_odds) HIPCHK(h, hipMemcpyAsync(log_odds, h->P.log_odds, m * C * sizeof(float), hipMemcpyDefault, h->stream));
    if (occ) HIPCHK(h, hipMemcpyAsync(occ, h->P.occ, m * C, hipMemcpyDefault, h->stream));
    if (infl) HIPCHK(h, hipMemcpyAsync(infl, h->P.infl, m * C, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

namespace {
constexpr unsigned int kWinFillGrid = 2048, kWinGradGrid = 8192; // most workgroups of mlm_export_window's kernels
} // namespace

int mlm_export_window(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int max_iter, float *odds, int8_t *occ, int8_t *infl,
                      double *grad3) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!lo || !dims || max_iter < 0 || (!odds && !occ && !infl && !grad3)) {
        h->err = "mlm_export_window: null window, negative max_iter or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_window", lo, dims, D, nvox);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    ReadoutChannels<4> ch(h->d_win_stage, {{odds, sizeof(float)}, {occ, 1}, {infl, 1}, {grad3, 3 * sizeof(double)}});
    // tiles as mlm_export_esdf's (C - 1 = H, the halo of the gradients): the haloed tile's odds take at most kEsdfBoxVoxels floats
    // (128 MB), a tile staged for host destinations at most kEsdfStageVoxels voxels (<= 30 bytes each); H <= MLM_WIN_HALO: a tile fits
    const long long H = grad3 ? std::min(max_iter, MLM_WIN_HALO) : 0;
    const MlmEsdfPlan plan = mlm_esdf_plan(D, (int)H + 1, false, grad3 ? kEsdfBoxVoxels : 1ll << 62, ch.any_staged ? kEsdfStageVoxels : 1ll << 62);
    const long long *T = plan.T;
    if (grad3 && (rc = readout_reserve(h, h->d_win_scratch, (size_t)plan.grown * sizeof(float), "mlm_export_window"))) return rc;
    if ((rc = ch.reserve(h, "mlm_export_window", (size_t)(T[0] * T[1] * T[2])))) return rc;

    rc = mlm_for_tiles(D, T, [&](const long long org[3], const int td[3], long long out_base) -> int {
        MlmWin W{};
        for (int a = 0; a < 3; ++a) {
            W.wlo[a] = lo[a];
            W.wd[a] = dims[a];
            W.tlo[a] = lo[a] + org[a];
            W.td[a] = td[a];
            W.hlo[a] = W.tlo[a] - H;
            W.hd[a] = W.td[a] + (int)(2 * H);
        }
        brick_cover(h, 3, W.hlo, W.hd, W.b0, W.nb);
        // (every channel pointer is where the tile's first voxel goes: out_base is the tile's index in the window)
        W.out_base = out_base;
        W.odds = (float *)ch.at(0, (size_t)out_base);
        W.occ = (int8_t *)ch.at(1, (size_t)out_base);
        W.infl = (int8_t *)ch.at(2, (size_t)out_base);
        W.grad = (double *)ch.at(3, (size_t)out_base);
        W.scratch = grad3 ? (float *)h->d_win_scratch.p : nullptr;
        W.halo = (int)H;
        W.max_iter = max_iter;
        launch(h, k_window_fill, bricks_grid((long long)W.nb[0] * W.nb[1] * W.nb[2], kWinFillGrid), 0, h->P, W);
        const long long nt = (long long)td[0] * td[1] * td[2];
        if (grad3) launch(h, k_window_grad, lanes_grid((size_t)nt, kWinGradGrid), 0, h->P, W);
        HIPCHK(h, hipGetLastError());
        return ch.copy_out(h, 0, 4, (size_t)out_base, (size_t)nt);
    });
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_export_esdf(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int max_dist, int flags, int32_t *sqdist, float *dist,
                    float *grad3) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!lo || !dims || max_dist < 1 || max_dist > 64 || (flags & 7) == 0 || (flags & ~15) || (!sqdist && !dist && !grad3)) {
        h->err = "mlm_export_esdf: null window, max_dist outside [1, 64], no obstacle bit or an unknown bit in flags, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_esdf", lo, dims, D, nvox);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    ReadoutChannels<3> ch(h->d_win_stage, {{sqdist, sizeof(int32_t)}, {dist, sizeof(float)}, {grad3, 3 * sizeof(float)}});
    const bool sgn = (flags & MLM_ESDF_SIGNED) != 0;
    const int C = max_dist, G = grad3 ? 1 : 0;
    long long box_cap = kEsdfBoxVoxels, kv;
    if (knob("esdf_tile_vox", kv)) box_cap = kv;
    const MlmEsdfPlan plan = mlm_esdf_plan(D, C, G != 0, box_cap, ch.any_staged ? kEsdfStageVoxels : (1ll << 62));
    if (plan.T[0] < 1) { // (not with the caps mlm_debug_set admits)
        h->err = "mlm_export_esdf: no tile fits the voxel cap";
        return MLM_ERR_INVALID;
    }
    // scratch: the mask, then two fields of the grown tile (the x pass and the z pass write the first, the y pass the second)
    const size_t fe = sgn ? 4 : 2, mask_bytes = mlm_align256((size_t)plan.grown), field_bytes = mlm_align256((size_t)plan.grown * fe);
    if ((rc = readout_reserve(h, h->d_esdf_scratch, mask_bytes + 2 * field_bytes, "mlm_export_esdf"))) return rc;
    if ((rc = ch.reserve(h, "mlm_export_esdf", (size_t)(plan.T[0] * plan.T[1] * plan.T[2])))) return rc;
    uint8_t *mask = (uint8_t *)h->d_esdf_scratch.p;
    void *fa = mask + mask_bytes, *fb = mask + mask_bytes + field_bytes;

    const long long H = plan.H;
    rc = mlm_for_tiles(D, plan.T, [&](const long long org[3], const int td[3], long long out_base) -> int {
        MlmEsdf E{};
        MlmEsdfOut Q{};
        for (int a = 0; a < 3; ++a) {
            Q.t0[a] = org[a];
            Q.td[a] = td[a];
            Q.fd[a] = Q.td[a] + 2 * G;
            E.glo[a] = lo[a] + org[a] - H;
            E.gd[a] = Q.td[a] + (int)(2 * H);
        }
        brick_cover(h, 3, E.glo, E.gd, E.b0, E.nb);
        E.flags = flags & 7;
        E.mask = mask;
        Q.wd0 = D[0];
        Q.wd1 = D[1];
        Q.G = G;
        Q.out_base = out_base;
        Q.d = (float)h->cfg.subbox_d_xyz;
        Q.inv = (float)(0.5 / h->cfg.subbox_d_xyz);
        Q.sqdist = (int32_t *)ch.at(0, (size_t)out_base);
        Q.dist = (float *)ch.at(1, (size_t)out_base);
        Q.grad = (float *)ch.at(2, (size_t)out_base);
        if (sgn)
            esdf_tile<true>(h, E, C, mask, fa, fb, Q);
        else
            esdf_tile<false>(h, E, C, mask, fa, fb, Q);
        HIPCHK(h, hipGetLastError());
        return ch.copy_out(h, 0, 3, (size_t)out_base, (size_t)td[0] * td[1] * td[2]);
    });
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_export_grid2d(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, int min_free, int z_ref, int max_dist,
                      int8_t *grid, int32_t *cols, int32_t *sqdist, float *dist, int64_t summary[6]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const bool want_dist = sqdist || dist;
    if (!lo || !dims || (flags & 7) == 0 || (flags & ~(7 | MLM_GRID_DIST_UNOBSERVED)) || (!grid && !cols && !sqdist && !dist && !summary)) {
        h->err = "mlm_export_grid2d: null window, no class bit or an unknown bit in flags, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_grid2d", lo, dims, D, nvox);
    if (rc) return rc;
    if (lo[2] == INT32_MIN || min_free < 0 || min_free > dims[2] || (cols && (z_ref < lo[2] || z_ref >= lo[2] + dims[2])) ||
        (want_dist && (max_dist < 1 || max_dist > 64))) {
        h->err = "mlm_export_grid2d: lo[2] == INT32_MIN, min_free outside [0, dims[2]], z_ref outside the slab or max_dist outside [1, 64]";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    ReadoutChannels<4> ch(h->d_win_stage, {{grid, 1}, {cols, MLM_GRID_COL * sizeof(int32_t)}, {sqdist, sizeof(int32_t)}, {dist, sizeof(float)}});
    const int C = want_dist ? max_dist : 1;
    long long out_cap = ch.any_staged ? kGridStageCells : (1ll << 62), kv;
    if (knob("grid_tile", kv)) out_cap = std::min(out_cap, kv);
    const MlmGridPlan plan = mlm_grid_plan(D, C, want_dist, kGridBoxCells, out_cap);
    if (plan.T[0] < 1) { // (not with the caps mlm_debug_set admits)
        h->err = "mlm_export_grid2d: no tile fits the cell cap";
        return MLM_ERR_INVALID;
    }
    // scratch: the summary counters, then (with distances) the mask and two u16 fields of the grown tile
    const size_t ctrl_bytes = 256, mask_bytes = want_dist ? mlm_align256((size_t)plan.grown) : 0,
                 field_bytes = want_dist ? mlm_align256((size_t)plan.grown * 2) : 0;
    if ((rc = readout_reserve(h, h->d_esdf_scratch, ctrl_bytes + mask_bytes + 2 * field_bytes, "mlm_export_grid2d"))) return rc;
    if ((rc = ch.reserve(h, "mlm_export_grid2d", (size_t)(plan.T[0] * plan.T[1])))) return rc;
    if (summary && (rc = ctrl_block(h))) return rc;
    char *base = (char *)h->d_esdf_scratch.p;
    unsigned long long *sums = summary ? (unsigned long long *)base : nullptr;
    uint8_t *mask = want_dist ? (uint8_t *)base + ctrl_bytes : nullptr;
    uint16_t *fa = (uint16_t *)(base + ctrl_bytes + mask_bytes), *fb = (uint16_t *)((char *)fa + field_bytes);
    if (sums) HIPCHK(h, hipMemsetAsync(sums, 0, 6 * sizeof(unsigned long long), h->stream));

    const int n = h->P.n;
    const long long H = plan.H;
    // a workgroup has one lane per column of a brick stack: whole waves, as many as a full brick's n^2 columns need
    const unsigned int block = (unsigned int)std::min<long long>(MLM_BLOCK, (((long long)n * n + 63) / 64) * 64);
    const long long plane[3] = {D[0], D[1], 1}, ptile[3] = {plan.T[0], plan.T[1], 1}; // (the tiles cut the plane; a tile is the whole slab in z)
    rc = mlm_for_tiles(plane, ptile, [&](const long long org[3], const int td[3], long long out_base) -> int {
        MlmGrid G{};
        for (int a = 0; a < 2; ++a) {
            G.tlo[a] = lo[a] + org[a];
            G.td[a] = td[a];
            G.glo[a] = G.tlo[a] - H;
            G.gd[a] = G.td[a] + (int)(2 * H);
        }
        brick_cover(h, 2, G.glo, G.gd, G.b0, G.nb);
        G.zlo = lo[2];
        G.zhi = lo[2] + dims[2];
        mlm_brick_cover(n, G.zlo, dims[2], G.b0[2], G.nb[2]);
        G.flags = flags;
        G.min_free = min_free;
        G.z_ref = z_ref;
        G.grid = (int8_t *)ch.at(0, (size_t)out_base); // (every channel pointer is where the tile's first cell goes)
        G.cols = (int32_t *)ch.at(1, (size_t)out_base);
        G.mask = mask;
        G.sums = sums;
        const dim3 cgrid(bricks_grid((long long)G.nb[0] * G.nb[1], kGridColGrid));
        if (cols)
            hipLaunchKernelGGL(k_grid_columns<true>, cgrid, dim3(block), 0, h->stream, h->P, G);
        else
            hipLaunchKernelGGL(k_grid_columns<false>, cgrid, dim3(block), 0, h->stream, h->P, G);
        const long long nt = (long long)G.td[0] * G.td[1];
        if (want_dist) {
            // x: mask [gd1][gd0] -> fa [gd1][td0];  y: fa -> fb [td1][td0]
            const long long rows = G.gd[1], xtasks = rows * ((G.td[0] + 63) / 64);
            launch(h, k_esdf_x<false>, bricks_grid((xtasks + 3) / 4, kEsdfPassGrid), 0, (const uint8_t *)mask, (void *)fa, rows, G.gd[0], G.td[0], C);
            const int lc = (G.td[1] + MLM_ESDF_LINE_TL - 1) / MLM_ESDF_LINE_TL, TL = (G.td[1] + lc - 1) / lc;
            const long long ltiles = (long long)lc * ((G.td[0] + 63) / 64);
            hipLaunchKernelGGL(k_esdf_line<uint16_t>, dim3((unsigned int)std::min<long long>(ltiles, kEsdfPassGrid)), dim3(MLM_BLOCK),
                               (size_t)(TL + 2 * C - 2) * 64 * sizeof(uint16_t), h->stream, (const uint16_t *)fa, fb, (long long)G.td[0], G.td[1],
                               1, C, TL);
            launch(h, k_grid_dist_out, lanes_grid((size_t)nt, kEsdfPassGrid), 0, (const uint16_t *)fb, nt, (float)h->cfg.subbox_d_xyz,
                   (int32_t *)ch.at(2, (size_t)out_base), (float *)ch.at(3, (size_t)out_base));
        }
        HIPCHK(h, hipGetLastError());
        return ch.copy_out(h, 0, 4, (size_t)out_base, (size_t)nt);
    });
    if (rc) return rc;
    return read_back(h, sums, summary ? 6 : 0, summary);
}

int mlm_export_reach(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], const int32_t *seeds3, int n_seeds, int flags, int clearance,
                     int max_steps, int32_t *steps, uint8_t *parent, int64_t summary[4]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!lo || !dims || !seeds3 || n_seeds < 1 || (flags & ~7) || clearance < 0 || clearance > 63 || max_steps < 1 ||
        (!steps && !parent && !summary)) {
        h->err = "mlm_export_reach: null window or seeds, n_seeds < 1, an unknown flag bit, clearance outside [0, 63], max_steps < 1 or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_reach", lo, dims, D, nvox);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    long long tile = kReachTileDefault, group = kReachGroupDefault, kv;
    if (knob("reach_tile", kv)) tile = kv;
    if (knob("reach_group", kv)) group = kv;
    const MlmReachPlan plan = mlm_reach_plan(D, tile, n_seeds, max_steps);
    if (!plan.ok) { // (not with the tiles mlm_debug_set admits)
        h->err = "mlm_export_reach: no such tile";
        return MLM_ERR_INVALID;
    }
    // outputs: written in place, or staged in ranges of the box
    ReadoutChannels<2> ch(h->d_win_stage, {{steps, sizeof(int32_t)}, {parent, 1}});
    const long long chunk = ch.any_staged ? std::min(nvox, kEsdfStageVoxels) : nvox;
    if ((rc = readout_reserve(h, h->d_reach, (size_t)plan.scratch_bytes, "mlm_export_reach"))) return rc;
    if ((rc = ch.reserve(h, "mlm_export_reach", (size_t)chunk))) return rc;
    if ((rc = ctrl_block(h))) return rc;
    char *base = (char *)h->d_reach.p;
    uint8_t *mask = (uint8_t *)(base + plan.off_mask), *dirty[2] = {(uint8_t *)(base + plan.off_dirty), (uint8_t *)(base + plan.off_dirty + plan.dirty_bytes)};
    unsigned int *marked = (unsigned int *)(base + plan.off_ctrl);
    unsigned long long *cnt = (unsigned long long *)(base + plan.off_ctrl + offsetof(MlmCtrlBlock, cnt));
    int32_t *seeds = (int32_t *)(base + plan.off_seeds);
    MlmReach R{};
    for (int a = 0; a < 3; ++a) {
        R.D[a] = D[a];
        R.n[a] = plan.n[a];
        R.T[a] = (int)plan.T[a];
    }
    R.tiles = plan.tiles;
    R.max_steps = (uint32_t)max_steps;
    R.field = (uint32_t *)base;

    // the blocked mask of the box
    if (clearance == 0) {
        mask_box(h, lo, dims, flags, mask);
    } else {
        // D_out <= clearance^2 of mlm_export_esdf at max_dist = clearance + 1
        rc = esdf_tiles(h, "mlm_export_reach", lo, D, clearance + 1, flags, [&](const uint16_t *fa, long long j0, long long nt) {
            launch(h, k_reach_blocked, lanes_grid((size_t)nt, kEsdfPassGrid), 0, fa, mask + j0, nt, (unsigned)(clearance * clearance));
        });
        if (rc) return rc;
    }
    // field, seeds, dirty arrays, control block
    HIPCHK(h, hipMemsetAsync(base + plan.off_dirty, 0, (size_t)(2 * plan.dirty_bytes + kReachCtrlBytes), h->stream));
    HIPCHK(h, hipMemcpyAsync(seeds, seeds3, (size_t)n_seeds * 12, hipMemcpyDefault, h->stream));
    launch(h, k_reach_init, lanes_grid((size_t)nvox, kReachGrid), 0, mask, R.field, nvox);
    launch(h, k_reach_seed, lanes_grid((size_t)n_seeds, 1024u), 0, R, (const int32_t *)seeds, n_seeds, (long long)lo[0], (long long)lo[1],
           (long long)lo[2], dirty[0]);
    HIPCHK(h, hipGetLastError());
    // sweeps in groups (settle): the dirty arrays swap roles from sweep to sweep
    const size_t lds = (size_t)(plan.T[0] + 2) * (plan.T[1] + 2) * (plan.T[2] + 2) * sizeof(uint32_t);
    const unsigned int sgrid = bricks_grid(plan.tiles, kReachGrid);
    const long long needed = settle(h, "mlm_export_reach", plan.cap, group, marked, [&](long long s, unsigned int *word) {
        launch(h, k_reach_sweep, sgrid, lds, R, dirty[s & 1], dirty[(s & 1) ^ 1], word);
    });
    if (needed < 0) return (int)needed;
    // outputs and counters
    rc = chunk_rounds(h, ch, (size_t)nvox, (size_t)chunk, 0, 0, 0, 2, [&](size_t j0, size_t m, void **at) {
        launch(h, k_reach_out, lanes_grid(m, kReachGrid), 0, R, (long long)j0, (long long)(j0 + m), (int32_t *)at[0], (uint8_t *)at[1], cnt);
        return MLM_OK;
    });
    if (rc) return rc;
    return settle_finish(h, cnt, needed, summary);
}

int mlm_export_route(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], const int32_t *seeds3, int n_seeds, int flags, int clearance,
                     int connectivity, const int32_t move_cost[3], const int32_t *penalty, int n_penalty, int max_cost, int32_t *cost,
                     uint8_t *parent, int64_t summary[4]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    bool ok = lo && dims && seeds3 && n_seeds >= 1 && !(flags & ~7) && clearance >= 0 && clearance <= 63 && mlm_route_connectivity_ok(connectivity) &&
              move_cost && n_penalty >= 0 && clearance + n_penalty <= 63 && (penalty || n_penalty == 0) && max_cost >= 1 && (cost || parent || summary);
    const int kinds = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; // (entries of move kinds the connectivity excludes are ignored)
    for (int k = 0; ok && k < kinds; ++k) ok = move_cost[k] >= 1 && move_cost[k] <= 65535;
    for (int k = 0; ok && k < n_penalty; ++k) ok = penalty[k] >= 0 && penalty[k] <= 65535;
    if (!ok) {
        h->err = "mlm_export_route: null window or seeds, n_seeds < 1, an unknown flag bit, clearance outside [0, 63], connectivity not 6 / 18 / 26, "
                 "move_cost NULL or an entry outside [1, 65535], n_penalty < 0, clearance + n_penalty > 63, penalty NULL with n_penalty > 0 or an "
                 "entry outside [0, 65535], max_cost < 1 or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_route", lo, dims, D, nvox);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    long long tile = kRouteTileDefault, group = kRouteGroupDefault, kv;
    if (knob("route_tile", kv)) tile = kv;
    if (knob("route_group", kv)) group = kv;
    const MlmRoutePlan plan = mlm_route_plan(D, tile, n_seeds);
    if (!plan.ok) { // (not with the tiles mlm_debug_set admits)
        h->err = "mlm_export_route: no such tile";
        return MLM_ERR_INVALID;
    }
    // outputs: written in place, or staged in ranges of the box
    ReadoutChannels<2> ch(h->d_win_stage, {{cost, sizeof(int32_t)}, {parent, 1}});
    const long long chunk = ch.any_staged ? std::min(nvox, kEsdfStageVoxels) : nvox;
    if ((rc = readout_reserve(h, h->d_reach, (size_t)plan.scratch_bytes, "mlm_export_route"))) return rc;
    if ((rc = ch.reserve(h, "mlm_export_route", (size_t)chunk))) return rc;
    if ((rc = ctrl_block(h))) return rc;
    char *base = (char *)h->d_reach.p;
    uint8_t *cls = (uint8_t *)(base + plan.off_class), *dirty[2] = {(uint8_t *)(base + plan.off_dirty), (uint8_t *)(base + plan.off_dirty + plan.dirty_bytes)};
    unsigned int *marked = (unsigned int *)(base + plan.off_ctrl);
    unsigned long long *cnt = (unsigned long long *)(base + plan.off_ctrl + offsetof(MlmCtrlBlock, cnt));
    uint32_t *pen = (uint32_t *)(base + plan.off_ctrl + offsetof(MlmCtrlBlock, pen));
    int32_t *seeds = (int32_t *)(base + plan.off_seeds);
    MlmRoute R{};
    for (int a = 0; a < 3; ++a) {
        R.D[a] = D[a];
        R.n[a] = plan.n[a];
        R.T[a] = (int)plan.T[a];
        R.move_cost[a] = a < kinds ? (uint32_t)move_cost[a] : 1u;
    }
    R.tiles = plan.tiles;
    R.connectivity = connectivity;
    R.max_cost = (uint32_t)max_cost;
    R.field = (uint32_t *)base;
    R.cls = cls;
    R.pen = pen;

    // the class bytes of the box
    if (clearance == 0 && n_penalty == 0) {
        mask_box(h, lo, dims, flags, cls);
    } else {
        // the rings of D_out of mlm_export_esdf at max_dist = clearance + n_penalty + 1
        rc = esdf_tiles(h, "mlm_export_route", lo, D, clearance + n_penalty + 1, flags, [&](const uint16_t *fa, long long j0, long long nt) {
            launch(h, k_route_class, lanes_grid((size_t)nt, kEsdfPassGrid), 0, fa, cls + j0, nt, clearance, n_penalty);
        });
        if (rc) return rc;
    }
    // field, seeds, dirty arrays, control block with the penalty table (staged in the pinned block behind what the host reads back)
    uint32_t *h_pen = h->h_ctrl->pen;
    for (int k = 0; k < kRoutePenWords; ++k) h_pen[k] = k < n_penalty ? (uint32_t)penalty[k] : 0u;
    HIPCHK(h, hipMemsetAsync(base + plan.off_dirty, 0, (size_t)(2 * plan.dirty_bytes + kReachCtrlBytes), h->stream));
    HIPCHK(h, hipMemcpyAsync(pen, h_pen, (size_t)kRoutePenWords * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(seeds, seeds3, (size_t)n_seeds * 12, hipMemcpyDefault, h->stream));
    launch(h, k_route_init, lanes_grid((size_t)nvox, kReachGrid), 0, (const uint8_t *)cls, R.field, nvox, n_penalty);
    launch(h, k_route_seed, lanes_grid((size_t)n_seeds, 1024u), 0, R, (const int32_t *)seeds, n_seeds, (long long)lo[0], (long long)lo[1],
           (long long)lo[2], dirty[0]);
    HIPCHK(h, hipGetLastError());
    // sweeps in groups, as mlm_export_reach runs them
    auto sweep = connectivity == 6 ? k_route_sweep<6> : connectivity == 18 ? k_route_sweep<18> : k_route_sweep<26>;
    const size_t lds = (size_t)plan.lds_bytes;
    if (lds > 65536) HIPCHK(h, hipFuncSetAttribute((const void *)sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned int sgrid = bricks_grid(plan.tiles, kReachGrid);
    const long long needed = settle(h, "mlm_export_route", plan.cap, group, marked, [&](long long s, unsigned int *word) {
        launch(h, sweep, sgrid, lds, R, dirty[s & 1], dirty[(s & 1) ^ 1], word);
    });
    if (needed < 0) return (int)needed;
    // outputs and counters
    rc = chunk_rounds(h, ch, (size_t)nvox, (size_t)chunk, 0, 0, 0, 2, [&](size_t j0, size_t m, void **at) {
        launch(h, k_route_out, lanes_grid(m, kReachGrid), 0, R, (long long)j0, (long long)(j0 + m), (int32_t *)at[0], (uint8_t *)at[1], cnt);
        return MLM_OK;
    });
    if (rc) return rc;
    return settle_finish(h, cnt, needed, summary);
}

int mlm_export_clusters(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, int connectivity, int min_size, int32_t *labels,
                        int64_t *table, int cap, int64_t summary[6]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const bool frontier = flags == MLM_CLUSTER_FRONTIER;
    const int nfwd = mlm_cluster_nfwd(connectivity);
    if (!lo || !dims || !(frontier || (flags >= 1 && flags <= 7)) || !nfwd || min_size < 1 || cap < 0 || (cap == 0) != (table == nullptr) ||
        (!labels && !table && !summary)) {
        h->err = "mlm_export_clusters: null window, flags neither MLM_CLUSTER_FRONTIER nor a union of the class bits, connectivity not 6 / 18 / 26, "
                 "min_size < 1, cap < 0, cap == 0 with a table or cap > 0 without one, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_clusters", lo, dims, D, nvox);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    long long tile = kClusterTileDefault, kv;
    if (knob("cluster_tile", kv)) tile = kv;
    ReadoutChannels<1> ch(h->d_win_stage, {{labels, sizeof(int32_t)}});
    const bool table_staged = table && !readout_in_place(table), labels_staged = ch.any_staged;
    const MlmClusterPlan plan = mlm_cluster_plan(D, tile, frontier, table_staged ? std::min<long long>(cap, nvox) : 0); // (K <= voxels)
    if (!plan.ok) { // (not with the tiles mlm_debug_set admits)
        h->err = "mlm_export_clusters: no such tile";
        return MLM_ERR_INVALID;
    }
    // labels: written in place, or staged through d_win_stage in ranges of the box (the one channel lies at the staging's start, and
    // its bytes are reserved as they are, not rounded as ch.reserve would); rows: in place, or in the scratch
    const long long chunk = labels_staged ? std::min(nvox, kEsdfStageVoxels) : nvox;
    if ((rc = readout_reserve(h, h->d_cluster, (size_t)plan.scratch_bytes, "mlm_export_clusters"))) return rc;
    if (labels_staged && (rc = readout_reserve(h, h->d_win_stage, (size_t)chunk * sizeof(int32_t), "mlm_export_clusters"))) return rc;
    if ((rc = ctrl_block(h))) return rc;
    char *base = (char *)h->d_cluster.p;
    uint8_t *mask = (uint8_t *)(base + plan.off_mask);
    unsigned int *chunk_cnt = (unsigned int *)(base + plan.off_chunk);
    unsigned long long *cnt = (unsigned long long *)(base + plan.off_ctrl);
    int64_t *rows = !table ? nullptr : table_staged ? (int64_t *)(base + plan.off_table) : table;
    MlmCluster R{};
    for (int a = 0; a < 3; ++a) {
        R.D[a] = D[a];
        R.lo[a] = lo[a];
        R.n[a] = plan.n[a];
        R.T[a] = (int)plan.T[a];
    }
    R.tiles = plan.tiles;
    R.nvox = nvox;
    R.nfwd = nfwd;
    R.min_size = (uint32_t)min_size;
    R.field = (uint32_t *)base;
    R.num = (uint32_t *)(base + plan.off_num);

    // the mask of the box
    const unsigned int vgrid = lanes_grid((size_t)nvox, kReachGrid);
    if (frontier) {
        MlmClusterOcc E{};
        for (int a = 0; a < 3; ++a) {
            E.glo[a] = (long long)lo[a] - 1;
            E.gd[a] = D[a] + 2;
        }
        brick_cover(h, 3, E.glo, E.gd, E.b0, E.nb);
        E.out = (uint8_t *)(base + plan.off_grown);
        launch(h, k_cluster_occ, bricks_grid((long long)E.nb[0] * E.nb[1] * E.nb[2], kEsdfMaskGrid), 0, h->P, E);
        launch(h, k_cluster_frontier, vgrid, 0, (const uint8_t *)E.out, mask, D[0], D[1], nvox);
    } else {
        mask_box(h, lo, dims, flags, mask);
    }
    HIPCHK(h, hipGetLastError());
    // local, merge, flatten and sizes, numbering
    HIPCHK(h, hipMemsetAsync(cnt, 0, (size_t)kClusterCtrlBytes, h->stream));
    const size_t lds = (size_t)plan.T[0] * plan.T[1] * plan.T[2] * sizeof(uint32_t);
    const unsigned int cgrid = bricks_grid(plan.chunks, kReachGrid);
    launch(h, k_cluster_local, bricks_grid(plan.tiles, kReachGrid), lds, R, (const uint8_t *)mask, cnt);
    launch(h, k_cluster_merge, vgrid, 0, R);
    launch(h, k_cluster_flatten, vgrid, 0, R, cnt);
    launch(h, k_cluster_count, cgrid, 0, R, plan.chunks, chunk_cnt, cnt);
    launch(h, k_cluster_scan, 1u, 0, chunk_cnt, plan.chunks, cnt);
    launch(h, k_cluster_rank, cgrid, 0, R, plan.chunks, (const unsigned int *)chunk_cnt, rows, cap);
    HIPCHK(h, hipGetLastError());
    // labels and rows
    if (labels || rows) {
        rc = chunk_rounds(h, ch, (size_t)nvox, (size_t)chunk, 0, 0, 0, 1, [&](size_t j0, size_t m, void **at) {
            launch(h, k_cluster_write, lanes_grid(m, kReachGrid), 0, R, (long long)j0, (long long)(j0 + m), (int32_t *)at[0], rows, cap);
            return MLM_OK;
        });
        if (rc) return rc;
    }
    int64_t sm[6] = {};
    if ((rc = read_back(h, cnt, summary || table_staged ? 6 : 0, sm))) return rc;
    if (table_staged) { // the rows that exist: min(K, cap)
        const size_t k = (size_t)std::min<unsigned long long>((unsigned long long)sm[2], (unsigned long long)cap);
        if (k) {
            HIPCHK(h, hipMemcpyAsync(table, rows, k * MLM_CLUSTER_ROW * sizeof(int64_t), hipMemcpyDefault, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
    }
    if (summary) std::copy(sm, sm + 6, summary);
    return MLM_OK;
}

int mlm_export_mesh(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, int32_t *quads, int32_t *face4, int64_t cap_faces,
                    int32_t *vert3, float *vert_xyz, int8_t *vert_n3, int64_t cap_verts, int64_t summary[MLM_MESH_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!lo || !dims || mlm_mesh_args(flags, cap_faces, quads || face4, cap_verts, vert3 || vert_xyz || vert_n3, summary != nullptr)) {
        h->err = "mlm_export_mesh: null window, none of MLM_MESH_OCC / _INFL / _UNKNOWN or an unknown flag bit, a negative cap, a cap of 0 with "
                 "one of its arrays or above 0 without any, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_mesh", lo, dims, D, nvox);
    if (rc) return rc;
    const MlmMeshPlan plan = mlm_mesh_plan(D);
    if (plan.why) {
        h->err = "mlm_export_mesh: more than 2^31 - 1 lattice points";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    // channels: quads, face4 (rows of faces), vert3, vert_xyz, vert_n3 (rows of vertices); in device memory (written in place) or
    // staged through d_win_stage in ranges of the numbering
    ReadoutChannels<5> ch(h->d_win_stage, {{quads, 4 * sizeof(int32_t)}, {face4, 4 * sizeof(int32_t)}, {vert3, 3 * sizeof(int32_t)},
                                           {vert_xyz, 3 * sizeof(float)}, {vert_n3, 3}});
    if ((rc = readout_reserve(h, h->d_mesh, (size_t)plan.scratch_bytes, "mlm_export_mesh"))) return rc;
    if ((rc = ctrl_block(h))) return rc;
    char *base = (char *)h->d_mesh.p;
    const long long lo64[3] = {lo[0], lo[1], lo[2]};
    const MlmMeshGeo G = mlm_mesh_geo(D, lo64, h->P.n, h->P.d_sub, h->P.d_glb, flags);
    MlmMeshArrays A{};
    A.state = (const uint8_t *)base;
    A.fmask = (uint8_t *)(base + plan.off_fmask);
    A.bits = (unsigned long long *)(base + plan.off_bits);
    A.wbase = (uint32_t *)(base + plan.off_wbase);
    A.fchunk = (unsigned long long *)(base + plan.off_fchunk);
    A.vchunk = (unsigned long long *)(base + plan.off_vchunk);
    A.cnt = (unsigned long long *)(base + plan.off_ctrl);
    A.fchunks = plan.fchunks;
    A.vchunks = plan.vchunks;

    // states of the grown box, masks, bits and chunk counts, chunk bases and the totals
    MlmMeshState E{};
    for (int a = 0; a < 3; ++a) {
        E.glo[a] = lo64[a] - 1;
        E.gd[a] = D[a] + 2;
    }
    brick_cover(h, 3, E.glo, E.gd, E.b0, E.nb);
    E.flags = flags;
    E.out = (uint8_t *)base;
    HIPCHK(h, hipMemsetAsync(A.cnt, 0, (size_t)kMeshCtrlBytes, h->stream));
    launch(h, k_mesh_state, bricks_grid((long long)E.nb[0] * E.nb[1] * E.nb[2], kEsdfMaskGrid), 0, h->P, E);
    const unsigned int fgrid = bricks_grid(plan.fchunks, kReachGrid), vgrid = bricks_grid(plan.vchunks, kReachGrid);
    launch(h, k_mesh_count, vgrid, 0, G, A); // (fchunks <= vchunks)
    launch(h, k_mesh_scan, 2u, 0, A);
    HIPCHK(h, hipGetLastError());
    int64_t sm[MLM_MESH_ROW];
    if ((rc = read_back(h, A.cnt, MLM_MESH_ROW, sm))) return rc;
    sm[11] = 0;

    // rows: the first min(F, cap_faces) faces and min(V, cap_verts) vertices, in ranges where a destination is staged; the word bases
    // that the quads read come with the vertices' launch
    const long long nF = std::min<long long>(sm[0], cap_faces), nV = std::min<long long>(sm[1], cap_verts);
    const bool faces_staged = ch.staged[0] || ch.staged[1], verts_staged = ch.staged[2] || ch.staged[3] || ch.staged[4];
    long long stage_rows = kMeshStageRows, kv;
    if (knob("mesh_stage_rows", kv)) stage_rows = kv;
    const long long fstep = faces_staged ? std::min(nF, stage_rows) : nF, vstep = verts_staged ? std::min(nV, stage_rows) : nV;
    const size_t stage_counts[5] = {(size_t)fstep, (size_t)fstep, (size_t)vstep, (size_t)vstep, (size_t)vstep};
    if ((rc = ch.reserve(h, "mlm_export_mesh", stage_counts))) return rc;
    if (nV > 0 || (quads && nF > 0)) {
        long long v0 = 0;
        do {
            const long long v1 = std::min(nV, v0 + vstep);
            const bool rows = v1 > v0;
            launch(h, k_mesh_verts, vgrid, 0, G, A, v0, v1, (int32_t *)(rows ? ch.at(2, (size_t)v0) : nullptr),
                   (float *)(rows ? ch.at(3, (size_t)v0) : nullptr), (int8_t *)(rows ? ch.at(4, (size_t)v0) : nullptr));
            HIPCHK(h, hipGetLastError());
            if ((rc = ch.copy_out(h, 2, 5, (size_t)v0, (size_t)(v1 - v0)))) return rc;
            v0 = v1;
        } while (v0 < nV);
    }
    rc = chunk_rounds(h, ch, (size_t)nF, (size_t)fstep, 0, 0, 0, 2, [&](size_t f0, size_t m, void **at) {
        launch(h, k_mesh_faces, fgrid, 0, G, A, (long long)f0, (long long)(f0 + m), (int32_t *)at[0], (int32_t *)at[1]);
        return MLM_OK;
    });
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (summary)
        for (int i = 0; i < MLM_MESH_ROW; ++i) summary[i] = sm[i];
    return MLM_OK;
}

int mlm_export_octree(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int depth, int flags, uint16_t *words, int32_t *inner4,
                      int32_t *skip, int64_t cap_inner, int32_t *leaf4, int8_t *leaf_class, int64_t cap_leaves, int64_t summary[MLM_OCT_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!lo || !dims || mlm_oct_args(flags, cap_inner, words || inner4 || skip, cap_leaves, leaf4 || leaf_class, summary != nullptr)) {
        h->err = "mlm_export_octree: null window, an unknown flag bit, a negative cap, a cap of 0 with one of its arrays or above 0 without "
                 "any, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_export_octree", lo, dims, D, nvox);
    if (rc) return rc;
    const long long lo64[3] = {lo[0], lo[1], lo[2]};
    const MlmOctPlan plan = mlm_oct_plan(lo64, D, depth);
    if (plan.why) {
        h->err = plan.why == 1 ? "mlm_export_octree: depth must be 1..31" : "mlm_export_octree: the box is not within [-2^(depth-1), 2^(depth-1)) per axis";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = drain(h))) return rc;

    // channels: words, inner4, skip (rows of inner nodes), leaf4, leaf_class (rows of leaves); in device memory (written in place) or
    // staged through d_win_stage in ranges of the numbering
    ReadoutChannels<5> ch(h->d_win_stage, {{words, sizeof(uint16_t)}, {inner4, 4 * sizeof(int32_t)}, {skip, sizeof(int32_t)},
                                           {leaf4, 4 * sizeof(int32_t)}, {leaf_class, 1}});
    if ((rc = readout_reserve(h, h->d_oct, (size_t)plan.scratch_bytes, "mlm_export_octree"))) return rc;
    if ((rc = ctrl_block(h))) return rc;
    const MlmOctGeo G = mlm_oct_geo(lo64, D, depth, flags, plan);
    const MlmOctUpper U = mlm_oct_upper(h->d_oct.p, plan);

    // up: the bricks, then the levels above them; down to the bricks; the counters
    const unsigned int bgrid = bricks_grid(plan.bricks, kOctGrid);
    HIPCHK(h, hipMemsetAsync(U.ctrl, 0, (size_t)kOctCtrlBytes, h->stream));
    launch(h, k_oct_up, bgrid, 0, h->P, G, U);
    launch(h, k_oct_tail, 1u, 0, G, U);
    HIPCHK(h, hipGetLastError());
    const unsigned long long *h_cnt;
    if ((rc = read_back(h, (const unsigned long long *)U.ctrl, kOctCtrlWords, h_cnt))) return rc;
    int64_t sm[MLM_OCT_ROW];
    mlm_oct_summary(h_cnt, sm);

    // rows: the first min(N, cap_inner) inner nodes and min(M, cap_leaves) leaves, in ranges where a destination is staged
    const long long nN = std::min<long long>(sm[0], cap_inner), nM = std::min<long long>(sm[1], cap_leaves);
    const bool inner_staged = ch.staged[0] || ch.staged[1] || ch.staged[2], leaves_staged = ch.staged[3] || ch.staged[4];
    const long long nstep = inner_staged ? std::min(nN, kOctStageRows) : nN, mstep = leaves_staged ? std::min(nM, kOctStageRows) : nM;
    const size_t stage_counts[5] = {(size_t)nstep, (size_t)nstep, (size_t)nstep, (size_t)mstep, (size_t)mstep};
    if ((rc = ch.reserve(h, "mlm_export_octree", stage_counts))) return rc;
    const long long upper_cells = plan.cells - plan.bricks;
    const unsigned int ugrid = std::max(1u, lanes_grid((size_t)upper_cells, kOctGrid));
    for (long long n0 = 0, m0 = 0; n0 < nN || m0 < nM;) {
        const long long n1 = std::min(nN, n0 + nstep), m1 = std::min(nM, m0 + mstep);
        MlmOctOut O{};
        if (n1 > n0) {
            O.words = (uint16_t *)ch.at(0, (size_t)n0);
            O.inner4 = (int32_t *)ch.at(1, (size_t)n0);
            O.skip = (int32_t *)ch.at(2, (size_t)n0);
        }
        if (m1 > m0) {
            O.leaf4 = (int32_t *)ch.at(3, (size_t)m0);
            O.leaf_class = (int8_t *)ch.at(4, (size_t)m0);
        }
        O.n0 = n0, O.n1 = n1, O.m0 = m0, O.m1 = m1;
        launch(h, k_oct_emit_upper, ugrid, 0, G, U, O);
        launch(h, k_oct_emit, bgrid, 0, h->P, G, U, O);
        HIPCHK(h, hipGetLastError());
        if (n1 > n0 && (rc = ch.copy_out(h, 0, 3, (size_t)n0, (size_t)(n1 - n0)))) return rc;
        if (m1 > m0 && (rc = ch.copy_out(h, 3, 5, (size_t)m0, (size_t)(m1 - m0)))) return rc;
        n0 = n1;
        m0 = m1;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (summary)
        for (int i = 0; i < MLM_OCT_ROW; ++i) summary[i] = sm[i];
    return MLM_OK;
}

int mlm_query_rays(mlm_handle *h, const double *p0, const double *p1, int n, int flags, int8_t *status, int32_t *voxel3, double *t,
                   int32_t *n_steps, int32_t *n_unknown) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n < 0 || (n > 0 && (!p0 || !p1)) || (flags & ~7) || (!status && !voxel3 && !t && !n_steps && !n_unknown)) {
        h->err = "mlm_query_rays: negative n, a null input, an unknown flag bit or no output";
        return MLM_ERR_INVALID;
    }
    if (n == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // channels: the two inputs, then the five outputs; bytes per ray; in device memory (used in place) or staged
    ReadoutChannels<7> ch(h->d_ray_stage,
                          {{p0, 3 * sizeof(double)}, {p1, 3 * sizeof(double)}, {status, 1}, {voxel3, 3 * sizeof(int32_t)}, {t, sizeof(double)},
                           {n_steps, sizeof(int32_t)}, {n_unknown, sizeof(int32_t)}},
                          true);
    // a planner's edge-by-edge calls: answered on the host (mlm_mirror.h), like run_query's small batches
    int rc = mirror_try(h, ch.all_host && mirror_rays_wanted(h, p0, p1, n), n, [&] { h->mir.view.rays(p0, p1, n, flags, status, voxel3, t, n_steps, n_unknown); });
    if (rc) return rc > 0 ? MLM_OK : rc;
    if ((rc = drain(h))) return rc;
    // chunks: staged channels of a chunk share one kept buffer (at most 77 bytes per ray)
    return for_chunks(h, ch, "mlm_query_rays", (size_t)n, (size_t)std::min(n, kRayChunk), 0, 2, 2, 7, [&](size_t, size_t m, void **at) {
        MlmRays R{(const double *)at[0], (const double *)at[1], (int)m, flags, (int8_t *)at[2], (int32_t *)at[3], (double *)at[4], (int32_t *)at[5], (int32_t *)at[6]};
        launch(h, k_rays, lanes_grid(m, h->rays_grid), 0, h->P, R);
        return MLM_OK;
    });
}

int mlm_render_depth(mlm_handle *h, const double *T_ws, int n_poses, int width, int height, const double K[4], int max_depth_mm, int flags,
                     uint16_t *depth, int8_t *status, int32_t *voxel3, int32_t *n_unknown, int64_t *table) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const double k4[4] = {K ? K[0] : h->cfg.cam_fx, K ? K[1] : h->cfg.cam_fy, K ? K[2] : h->cfg.cam_cx, K ? K[3] : h->cfg.cam_cy};
    const bool dims_ok = width >= 1 && width <= 8192 && height >= 1 && height <= 8192;
    const long long pixels = dims_ok && n_poses > 0 ? (long long)n_poses * width * height : 0;
    if (n_poses < 0 || (n_poses > 0 && !T_ws) || !dims_ok || pixels > 0x7FFFFFFFll || !(std::isfinite(k4[0]) && k4[0] > 0.0) ||
        !(std::isfinite(k4[1]) && k4[1] > 0.0) || !std::isfinite(k4[2]) || !std::isfinite(k4[3]) || max_depth_mm < 1 || max_depth_mm > 65535 ||
        (flags & ~7) || (!depth && !status && !voxel3 && !n_unknown && !table)) {
        h->err = "mlm_render_depth: negative n_poses, null poses, width or height outside 1..8192, more than 2^31 - 1 pixels, intrinsics not finite "
                 "or a focal length <= 0, max_depth_mm outside 1..65535, an unknown flag bit or no output";
        return MLM_ERR_INVALID;
    }
    if (n_poses == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc) return rc;
    // tiles; chunks of whole tile rows (counted over all poses: pose * tiles_y + ty), whose pixels are one contiguous range of the outputs
    const int TW = h->render_tile == 0 ? 64 : (h->render_tile == 1 ? 16 : 8), TH = 64 / TW;
    void (*const kern)(const MlmDev, const MlmRender) = TW == 64 ? k_render<64, 1> : (TW == 16 ? k_render<16, 4> : k_render<8, 8>);
    const int tiles_x = (width + TW - 1) / TW, tiles_y = (height + TH - 1) / TH;
    const long long q_total = (long long)n_poses * tiles_y; // (<= pixels)
    const long long q_chunk = std::max(1, kRenderChunk / (TH * width));
    const long long chunk_pixels = std::min(pixels, q_chunk * TH * width);
    auto first_pixel = [&](long long q) { return ((q / tiles_y) * height + (q % tiles_y) * TH) * width; };
    // channels: the poses, the four per-pixel outputs, the table; in device memory (used in place) or staged — poses and table for the
    // whole call, the per-pixel outputs chunk by chunk (at most 19 bytes per pixel)
    ReadoutChannels<6> ch(h->d_ray_stage,
                          {{T_ws, 12 * sizeof(double)}, {depth, sizeof(uint16_t)}, {status, 1}, {voxel3, 3 * sizeof(int32_t)},
                           {n_unknown, sizeof(int32_t)}, {table, MLM_RENDER_ROW * sizeof(int64_t)}},
                          true);
    const size_t np = (size_t)n_poses, cp = (size_t)chunk_pixels;
    if ((rc = ch.reserve(h, "mlm_render_depth", {np, cp, cp, cp, cp, np}))) return rc;
    if ((rc = ch.copy_in(h, 0, 1, 0, np))) return rc;
    if (table) HIPCHK(h, hipMemsetAsync(ch.at(5, 0), 0, np * ch.elem[5], h->stream));
    MlmRender R{};
    R.T = (const double *)ch.at(0, 0);
    for (int k = 0; k < 4; ++k) R.K[k] = k4[k];
    R.Z = (double)max_depth_mm / 1000.0;
    R.width = width, R.height = height, R.max_mm = max_depth_mm, R.flags = flags;
    R.tiles_x = tiles_x, R.tiles_y = tiles_y;
    R.table = (unsigned long long *)ch.at(5, 0);
    for (long long q0 = 0; q0 < q_total; q0 += q_chunk) {
        const long long q1 = std::min(q_total, q0 + q_chunk), i0 = first_pixel(q0), m = first_pixel(q1) - i0;
        void *at[5];
        for (int c = 1; c < 5; ++c) at[c] = ch.at(c, (size_t)i0);
        R.q0 = (int)q0, R.n_tiles = (int)((q1 - q0) * tiles_x), R.pix0 = i0;
        R.depth = (uint16_t *)at[1], R.status = (int8_t *)at[2], R.voxel3 = (int32_t *)at[3], R.n_unknown = (int32_t *)at[4];
        // one wave per tile, four to a workgroup
        launch(h, kern, wave_grid((size_t)R.n_tiles), 0, h->P, R);
        HIPCHK(h, hipGetLastError());
        if ((rc = ch.copy_out(h, 1, 5, (size_t)i0, (size_t)m))) return rc;
    }
    if ((rc = ch.copy_out(h, 5, 6, 0, np))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_query_boxes(mlm_handle *h, const int32_t *box6, int n, int flags, const int32_t max_grow[6], const int32_t lo[3], const int32_t dims[3],
                    int8_t *status, int32_t *out6, uint8_t *closed, int64_t *table) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n < 0 || (n > 0 && !box6) || (flags & ~7) || (!lo != !dims) || (!status && !out6 && !closed && !table)) {
        h->err = "mlm_query_boxes: negative n, a null box6, an unknown flag bit, lo without dims or no output";
        return MLM_ERR_INVALID;
    }
    MlmBoxLimits L{};
    for (int c = 0; c < 6; ++c) {
        L.grow[c] = max_grow ? max_grow[c] : 0;
        if (L.grow[c] < 0 || L.grow[c] > MLM_BOX_MAX_GROW) {
            h->err = "mlm_query_boxes: max_grow must lie in [0, 4096]";
            return MLM_ERR_INVALID;
        }
    }
    if (lo) {
        L.on = 1;
        long long D[3], nvox;
        if (int rc = box_check(h, "mlm_query_boxes", lo, dims, D, nvox)) return rc;
        for (int a = 0; a < 3; ++a) {
            L.wlo[a] = lo[a];
            L.whi[a] = lo[a] + (dims[a] - 1);
        }
    }
    if (n == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // channels: the input, then the four outputs; bytes per box; in device memory (used in place) or staged
    ReadoutChannels<5> ch(h->d_ray_stage,
                          {{box6, 6 * sizeof(int32_t)}, {status, 1}, {out6, 6 * sizeof(int32_t)}, {closed, 1}, {table, MLM_BOX_ROW * sizeof(int64_t)}}, true);
    // a planner's waypoint-by-waypoint calls: answered on the host (mlm_mirror.h), like mlm_query_rays' small batches
    int rc = mirror_try(h, ch.all_host && mirror_boxes_wanted(h, box6, n, L), n, [&] { h->mir.view.boxes(box6, n, flags, L, status, out6, closed, table); });
    if (rc) return rc > 0 ? MLM_OK : rc;
    if ((rc = drain(h))) return rc;
    // chunks: staged channels of a chunk share one kept buffer (at most 82 bytes per box)
    return for_chunks(h, ch, "mlm_query_boxes", (size_t)n, (size_t)std::min(n, kBoxChunk), 0, 1, 1, 5, [&](size_t, size_t m, void **at) {
        MlmBoxes B{(const int32_t *)at[0], (int)m, flags, L, (int8_t *)at[1], (int32_t *)at[2], (uint8_t *)at[3], (int64_t *)at[4]};
        // one wave per box, four to a workgroup; at most kBoxGrid workgroups (grid-stride)
        launch(h, k_boxes, wave_grid(m, kBoxGrid), 0, h->P, B);
        return MLM_OK;
    });
}

int mlm_query_nearest(mlm_handle *h, const double *pos, int n, int max_dist, int flags, int8_t *status, int32_t *voxel3, int32_t *delta3,
                      int64_t *sq, double *dist) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n < 0 || (n > 0 && !pos) || (flags & ~7) || !(flags & 7) || max_dist < 1 || max_dist > MLM_NEAR_MAX_DIST ||
        (!status && !voxel3 && !delta3 && !sq && !dist)) {
        h->err = "mlm_query_nearest: negative n, a null pos, no class bit or an unknown flag bit, max_dist outside [1, 64] or no output";
        return MLM_ERR_INVALID;
    }
    if (n == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // channels: the input, then the five outputs; bytes per point; in device memory (used in place) or staged
    ReadoutChannels<6> ch(h->d_ray_stage,
                          {{pos, 3 * sizeof(double)}, {status, 1}, {voxel3, 3 * sizeof(int32_t)}, {delta3, 3 * sizeof(int32_t)}, {sq, sizeof(int64_t)},
                           {dist, sizeof(double)}},
                          true);
    // an optimiser's few control points: answered on the host (mlm_mirror.h), like mlm_query_boxes' small batches
    int rc = mirror_try(h, ch.all_host && mirror_nearest_wanted(h, n, max_dist), n, [&] { h->mir.view.nearest(pos, n, max_dist, flags, status, voxel3, delta3, sq, dist); });
    if (rc) return rc > 0 ? MLM_OK : rc;
    if ((rc = drain(h))) return rc;
    // chunks: staged channels of a chunk share one kept buffer (at most 65 bytes per point)
    return for_chunks(h, ch, "mlm_query_nearest", (size_t)n, (size_t)std::min(n, kNearChunk), 0, 1, 1, 6, [&](size_t, size_t m, void **at) {
        MlmNearest Q{(const double *)at[0], (int)m, max_dist, flags, (int8_t *)at[1], (int32_t *)at[2], (int32_t *)at[3], (int64_t *)at[4], (double *)at[5]};
        // one wave per point, four to a workgroup; at most kNearGrid workgroups (grid-stride)
        launch(h, k_nearest, wave_grid(m, kNearGrid), 0, h->P, Q);
        return MLM_OK;
    });
}

int mlm_query_sweeps(mlm_handle *h, const double *p0, const double *p1, int n, int radius, int flags, int8_t *status, int32_t *voxel3, double *t,
                     int32_t *n_steps, int32_t *n_unknown, int32_t *hit3, int32_t *hit_sq) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n < 0 || (n > 0 && (!p0 || !p1)) || (flags & ~7) || radius < 0 || radius > MLM_SWEEP_MAX_RADIUS ||
        (!status && !voxel3 && !t && !n_steps && !n_unknown && !hit3 && !hit_sq)) {
        h->err = "mlm_query_sweeps: negative n, a null input, an unknown flag bit, radius outside [0, 16] or no output";
        return MLM_ERR_INVALID;
    }
    if (n == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // channels: the two inputs, then the seven outputs; bytes per ray; in device memory (used in place) or staged
    ReadoutChannels<9> ch(h->d_ray_stage,
                          {{p0, 3 * sizeof(double)}, {p1, 3 * sizeof(double)}, {status, 1}, {voxel3, 3 * sizeof(int32_t)}, {t, sizeof(double)},
                           {n_steps, sizeof(int32_t)}, {n_unknown, sizeof(int32_t)}, {hit3, 3 * sizeof(int32_t)}, {hit_sq, sizeof(int32_t)}},
                          true);
    // a planner's edge-by-edge calls: answered on the host (mlm_mirror.h), like mlm_query_rays' small batches
    int rc = mirror_try(h, ch.all_host && mirror_sweeps_wanted(h, p0, p1, n, radius), n, [&] { h->mir.view.sweep(p0, p1, n, radius, flags, status, voxel3, t, n_steps, n_unknown, hit3, hit_sq); });
    if (rc) return rc > 0 ? MLM_OK : rc;
    if ((rc = drain(h))) return rc;
    // chunks: staged channels of a chunk share one kept buffer (at most 93 bytes per ray)
    // the slots of the block box around the ball stay in LDS while the box has at most kSweepNB blocks per axis (mlm_kernels_sweeps.h)
    const bool cached = radius > 0 && (2 * radius - 1) / h->P.n + 2 <= kSweepNB;
    return for_chunks(h, ch, "mlm_query_sweeps", (size_t)n, (size_t)std::min(n, kSweepChunk), 0, 2, 2, 9, [&](size_t, size_t m, void **at) {
        MlmSweeps R{(const double *)at[0], (const double *)at[1], (int)m, radius, flags, mlm_sweep_columns(radius), (int8_t *)at[2], (int32_t *)at[3],
                    (double *)at[4], (int32_t *)at[5], (int32_t *)at[6], (int32_t *)at[7], (int32_t *)at[8]};
        if (radius == 0) // one lane per ray, as k_rays
            launch(h, k_sweeps0, lanes_grid(m, h->rays_grid), 0, h->P, R);
        else // one wave per ray, four to a workgroup; at most kSweepGrid workgroups (grid-stride)
            launch(h, cached ? k_sweeps<true> : k_sweeps<false>, wave_grid(m, kSweepGrid), 0, h->P, R);
        return MLM_OK;
    });
}

int mlm_query_paths(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], const uint8_t *parent, int kind, const int32_t *goals3, int n,
                    int lookahead, int max_moves, int cap, int8_t *status, int32_t *way3, double *length, int64_t *table) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!lo || !dims || !parent || (kind != MLM_PATH_REACH && kind != MLM_PATH_ROUTE) || n < 0 || (n > 0 && !goals3) || lookahead < 1 ||
        lookahead > MLM_PATH_MAX_LOOKAHEAD || max_moves < 1 || max_moves > MLM_PATH_MAX_MOVES || cap < 0 || (cap == 0) != (way3 == nullptr) ||
        (!status && !way3 && !length && !table)) {
        h->err = "mlm_query_paths: null window or parent, kind not 0 / 1, negative n, null goals, lookahead outside [1, 4096], max_moves outside "
                 "[1, 2^20], cap negative or at odds with way3, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox;
    int rc = box_check(h, "mlm_query_paths", lo, dims, D, nvox);
    if (rc) return rc;
    if (n == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const MlmPathField F{parent, {dims[0], dims[1], dims[2]}, mlm_path_seed_code(kind)};
    const double d = (double)(float)h->P.d_sub;
    // channels: the goals, then the four outputs; bytes per goal; way3 is read too (rows beyond W keep their content)
    ReadoutChannels<5> chs(h->d_ray_stage,
                           {{goals3, 3 * sizeof(int32_t)}, {status, 1}, {way3, (size_t)cap * 3 * sizeof(int32_t)}, {length, sizeof(double)},
                            {table, MLM_PATH_ROW * sizeof(int64_t)}},
                           true);

    if (!readout_in_place(parent)) {
        void *const *ch = chs.ptr;
        const size_t *elem = chs.elem;
        bool on_dev[5];
        for (int c = 0; c < 5; ++c) on_dev[c] = ch[c] && !chs.staged[c];
        // the field is in host memory: the shared rule on the host, no launch and no copy of the field; goals and outputs in device
        // memory are copied across
        std::vector<std::vector<char>> tmp(5);
        void *at[5];
        for (int c = 0; c < 5; ++c) {
            at[c] = ch[c];
            if (!on_dev[c]) continue;
            tmp[c].resize((size_t)n * elem[c]);
            at[c] = tmp[c].data();
            if (c == 0 || c == 2) HIPCHK(h, hipMemcpyAsync(at[c], ch[c], tmp[c].size(), hipMemcpyDeviceToHost, h->stream));
        }
        if (on_dev[0] || on_dev[2]) HIPCHK(h, hipStreamSynchronize(h->stream));
        const size_t len = (size_t)max_moves + 1;
        std::unique_ptr<int32_t[]> path(new (std::nothrow) int32_t[3 * len]); // (not touched beyond the longest path)
        if (!path) {
            h->err = "mlm_query_paths: no host memory for the path";
            return MLM_ERR_CAPACITY;
        }
        MlmPathSerial X{path.get(), path.get() + len, path.get() + 2 * len};
        for (int i = 0; i < n; ++i) {
            const MlmPathOut o{at[1] ? (int8_t *)at[1] + i : nullptr, at[2] ? (int32_t *)at[2] + 3 * (size_t)i * (size_t)cap : nullptr,
                               at[3] ? (double *)at[3] + i : nullptr, at[4] ? (int64_t *)at[4] + (size_t)i * MLM_PATH_ROW : nullptr};
            mlm_path_goal(F, lo, (const int32_t *)at[0] + 3 * (size_t)i, lookahead, max_moves, cap, d, X, o);
        }
        bool copied = false;
        for (int c = 1; c < 5; ++c)
            if (on_dev[c]) {
                HIPCHK(h, hipMemcpyAsync(ch[c], at[c], tmp[c].size(), hipMemcpyHostToDevice, h->stream));
                copied = true;
            }
        if (copied) HIPCHK(h, hipStreamSynchronize(h->stream));
        return MLM_OK;
    }

    // the field is in device memory: k_paths, a wave per goal.  Chunks of goals: the path scratch of a chunk (12 bytes x (max_moves + 1)
    // per goal) takes at most kPathScratchBytes, its staged host channels at most kPathStageBytes, and it has at most kPathChunk goals
    const size_t per_goal = 3 * sizeof(int32_t) * ((size_t)max_moves + 1);
    const size_t stage_per_goal = chs.staged_elem_bytes();
    size_t chunk = std::min<size_t>({(size_t)n, (size_t)kPathChunk, std::max<size_t>(1, kPathScratchBytes / per_goal)});
    if (stage_per_goal) chunk = std::min(chunk, std::max<size_t>(1, kPathStageBytes / stage_per_goal));
    if ((rc = readout_reserve(h, h->d_path, chunk * per_goal, "mlm_query_paths"))) return rc;
    return for_chunks(h, chs, "mlm_query_paths", (size_t)n, chunk, 0, 1, 1, 5, [&](size_t i0, size_t m, void **at) -> int {
        if (int rc2 = chs.copy_in(h, 2, 3, i0, m)) return rc2; // way3 in as well, for the rows the kernel leaves as they were
        MlmPaths Q{F, {lo[0], lo[1], lo[2]}, (const int32_t *)at[0], (int)m, lookahead, max_moves, cap, d, (int32_t *)h->d_path.p,
                   (int8_t *)at[1], (int32_t *)at[2], (double *)at[3], (int64_t *)at[4]};
        // one wave per goal and scratch slot, four to a workgroup (m <= kPathChunk: at most 16 384 workgroups)
        launch(h, k_paths, wave_grid(m), 0, Q);
        return MLM_OK;
    });
}

int mlm_score_poses(mlm_handle *h, const double *pts_s, int n_pts, const double *T_ws, int n_poses, int flags, const int32_t lo[3],
                    const int32_t dims[3], const int32_t *sqdist, int sq_cap, int64_t *table) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const bool classes = (flags & MLM_SCORE_CLASSES) != 0, field = lo || dims || sqdist;
    if (n_pts < 0 || n_pts > MLM_SCORE_MAX_COUNT || n_poses < 0 || n_poses > MLM_SCORE_MAX_COUNT || (n_pts > 0 && !pts_s) || (n_poses > 0 && !T_ws) ||
        !table || (flags & ~MLM_SCORE_CLASSES) || (!classes && !field) || (field && (!lo || !dims || !sqdist)) ||
        (field && (sq_cap < 1 || sq_cap > MLM_SCORE_MAX_CAP))) {
        h->err = "mlm_score_poses: n_pts or n_poses outside [0, 2^22], a null input, a null table, an unknown flag bit, neither classes nor a field, "
                 "lo / dims / sqdist only partly given, or sq_cap outside [1, 2^20]";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox = 0;
    int rc;
    if (field && (rc = box_check(h, "mlm_score_poses", lo, dims, D, nvox))) return rc;
    if (n_poses == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    MlmScoreField F{};
    if (field) {
        F.sqdist = sqdist;
        for (int a = 0; a < 3; ++a) F.lo[a] = lo[a], F.dims[a] = dims[a];
        F.cap = sq_cap;
    }
    // channels: the points, the poses, the rows; in device memory (used in place) or staged — the points for the whole call, poses and
    // rows chunk by chunk
    ReadoutChannels<3> ch(h->d_ray_stage,
                          {{pts_s, 3 * sizeof(double)}, {T_ws, 12 * sizeof(double)}, {table, MLM_SCORE_ROW * sizeof(int64_t)}}, true);
    const bool field_staged = field && !readout_in_place(sqdist);
    // a matcher's few hypotheses: answered on the host like mlm_query_nearest's small batches — from the host mirror (mlm_mirror.h) with
    // classes, with no mirror and no look at the map without
    if (ch.all_host && (!field || field_staged) && mirror_score_wanted(h, n_poses, n_pts)) {
        if (classes) {
            rc = mirror_try(h, true, n_poses, [&] { h->mir.view.score(pts_s, n_pts, T_ws, n_poses, true, F, table); });
            if (rc) return rc > 0 ? MLM_OK : rc;
        } else {
            mlm_host::MapView v;
            v.d_sub = h->P.d_sub;
            v.n = h->P.n;
            v.score(pts_s, n_pts, T_ws, n_poses, false, F, table);
            return MLM_OK;
        }
    }
    // with classes the call observes the map as queries do; a field-only call reads nothing of it and waits for nothing
    if (classes && (rc = drain(h))) return rc;
    if (field_staged) { // the field crosses the link once, into a buffer of its own
        const size_t bytes = (size_t)nvox * sizeof(int32_t);
        if ((rc = readout_reserve(h, h->d_score_field, bytes, "mlm_score_poses"))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_score_field.p, sqdist, bytes, hipMemcpyHostToDevice, h->stream));
        F.sqdist = (const int32_t *)h->d_score_field.p;
    }
    const int pose_chunk = std::min(n_poses, kScorePoseChunk);
    if ((rc = ch.reserve(h, "mlm_score_poses", {(size_t)n_pts, (size_t)pose_chunk, (size_t)pose_chunk}))) return rc;
    if ((rc = ch.copy_in(h, 0, 1, 0, (size_t)n_pts))) return rc;
    void (*const kern)(const MlmDev, const MlmScore) = classes ? (field ? k_score<true, true> : k_score<true, false>) : k_score<false, true>;
    const int tiles = std::max(1, (n_pts + MLM_SCORE_TILE - 1) / MLM_SCORE_TILE);
    for (int i0 = 0; i0 < n_poses; i0 += pose_chunk) {
        const int m = std::min(pose_chunk, n_poses - i0);
        const int groups = (m + MLM_BLOCK - 1) / MLM_BLOCK;
        // points per chunk: the knob's, else as many chunks as bring the grid to kScoreGridTarget workgroups, whole tiles each
        int chunk = h->score_chunk;
        if (chunk <= 0) {
            const int want = (int)std::min<long long>(tiles, (kScoreGridTarget + groups - 1) / groups);
            chunk = (tiles + want - 1) / want * MLM_SCORE_TILE;
        }
        const int chunks = std::max(1, (n_pts + chunk - 1) / chunk);
        if ((rc = ch.copy_in(h, 1, 2, (size_t)i0, (size_t)m))) return rc;
        MlmScore Q{(const double *)ch.at(0, 0), (const double *)ch.at(1, (size_t)i0), n_pts, m, chunk, chunks > 1, F, (unsigned long long *)ch.at(2, (size_t)i0)};
        if (chunks > 1) HIPCHK(h, hipMemsetAsync(Q.table, 0, (size_t)m * MLM_SCORE_ROW * sizeof(int64_t), h->stream));
        hipLaunchKernelGGL(kern, dim3((unsigned int)chunks, (unsigned int)groups), dim3(MLM_BLOCK), 0, h->stream, h->P, Q);
        HIPCHK(h, hipGetLastError());
        if ((rc = ch.copy_out(h, 2, 3, (size_t)i0, (size_t)m))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_query_clearance(mlm_handle *h, const double *p0, const double *p1, int n, const int32_t lo[3], const int32_t dims[3], const int32_t *sqdist,
                        int sq_stop, int sq_cap, int flags, int8_t *status, int32_t *voxel3, double *t, int32_t *n_steps, int32_t *min_sq,
                        int32_t *min3, int64_t *cost, int32_t *n_near, const int32_t *group_begin, int n_groups, int64_t *table) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n < 0 || (n > 0 && (!p0 || !p1)) || !lo || !dims || !sqdist || sq_stop < -1 || sq_stop > MLM_CLEAR_MAX_SQ || sq_cap < 1 ||
        sq_cap > MLM_CLEAR_MAX_SQ || (flags & ~MLM_CLEAR_OUTSIDE_PASS) || (!group_begin != !table) || n_groups < 0 ||
        (!status && !voxel3 && !t && !n_steps && !min_sq && !min3 && !cost && !n_near && !table)) {
        h->err = "mlm_query_clearance: negative n, a null input, a null lo, dims or sqdist, sq_stop outside [-1, 2^20], sq_cap outside [1, 2^20], an "
                 "unknown flag bit, group_begin without table or table without group_begin, negative n_groups, or no output";
        return MLM_ERR_INVALID;
    }
    long long D[3], nvox = 0;
    int rc = box_check(h, "mlm_query_clearance", lo, dims, D, nvox);
    if (rc) return rc;
    const bool grouped = table != nullptr;
    if (n == 0 && (!grouped || n_groups == 0)) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // group_begin: validated on the host (copied back when it is device memory, behind the caller's work on the stream)
    std::vector<int32_t> gb_copy;
    const int32_t *gb = group_begin;
    const bool gb_dev = grouped && readout_in_place(group_begin);
    if (gb_dev) {
        gb_copy.resize((size_t)n_groups + 1);
        HIPCHK(h, hipMemcpyAsync(gb_copy.data(), group_begin, gb_copy.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        gb = gb_copy.data();
    }
    if (grouped) {
        bool ok = gb[0] >= 0;
        for (int g = 0; g < n_groups && ok; ++g) ok = gb[g + 1] >= gb[g];
        if (!ok || gb[n_groups] > n) {
            h->err = "mlm_query_clearance: group_begin must start at >= 0, must not decrease and must end at <= n";
            return MLM_ERR_INVALID;
        }
    }
    MlmClearField F{};
    F.sqdist = sqdist;
    for (int a = 0; a < 3; ++a) F.lo[a] = lo[a], F.dims[a] = dims[a];
    F.sq_stop = sq_stop, F.sq_cap = sq_cap, F.outside_pass = (flags & MLM_CLEAR_OUTSIDE_PASS) ? 1 : 0;
    const double d = h->P.d_sub;
    // channels: the two inputs, then the eight per-ray outputs; bytes per ray; in device memory (used in place) or staged
    ReadoutChannels<10> ch(h->d_ray_stage,
                           {{p0, 3 * sizeof(double)}, {p1, 3 * sizeof(double)}, {status, 1}, {voxel3, 3 * sizeof(int32_t)}, {t, sizeof(double)},
                            {n_steps, sizeof(int32_t)}, {min_sq, sizeof(int32_t)}, {min3, 3 * sizeof(int32_t)}, {cost, sizeof(int64_t)},
                            {n_near, sizeof(int32_t)}},
                           true);
    const bool field_staged = !readout_in_place(sqdist), table_staged = grouped && !readout_in_place(table);

    // a planner's edge-by-edge calls: the shared rule on the host, no launch and no copy (no mirror either: the call reads no map state)
    bool on_host = ch.all_host && field_staged && (!grouped || (!gb_dev && table_staged)) && n <= kClearHostRays && h->mir.enabled;
    if (on_host) {
        long long vox = 0;
        for (int i = 0; i < n; ++i) {
            MlmRayState S;
            if (!mlm_ray_setup(p0 + 3 * (size_t)i, p1 + 3 * (size_t)i, d, 1, S)) continue;
            vox += 1 + (long long)S.r[0] + S.r[1] + S.r[2];
        }
        on_host = vox <= kClearHostVoxels;
    }
    if (on_host) {
        int8_t w_status[kClearHostRays];
        int32_t w_min[kClearHostRays], w_steps[kClearHostRays], w_near[kClearHostRays];
        int64_t w_cost[kClearHostRays];
        for (int i = 0; i < n; ++i) {
            MlmClearResult o;
            mlm_clear_walk<1>(p0 + 3 * (size_t)i, p1 + 3 * (size_t)i, d, F, o);
            w_status[i] = (int8_t)o.status, w_min[i] = o.min_sq, w_steps[i] = o.n_steps, w_near[i] = o.n_near, w_cost[i] = (int64_t)o.cost;
            if (status) status[i] = (int8_t)o.status;
            if (t) t[i] = o.t;
            if (n_steps) n_steps[i] = o.n_steps;
            if (min_sq) min_sq[i] = o.min_sq;
            if (cost) cost[i] = (int64_t)o.cost;
            if (n_near) n_near[i] = o.n_near;
            for (int a = 0; a < 3; ++a) {
                if (voxel3) voxel3[3 * (size_t)i + a] = o.voxel[a];
                if (min3) min3[3 * (size_t)i + a] = o.min3[a];
            }
        }
        for (int g = 0; grouped && g < n_groups; ++g)
            mlm_clear_group(gb[g], gb[g + 1], w_status, w_min, w_cost, w_steps, w_near, table + (size_t)g * MLM_CLEAR_WORDS);
        h->mir.n_host_queries += n;
        return MLM_OK;
    }

    if (field_staged) { // the field crosses the link once, into the buffer mlm_score_poses keeps for its field
        const size_t bytes = (size_t)nvox * sizeof(int32_t);
        if ((rc = readout_reserve(h, h->d_score_field, bytes, "mlm_query_clearance"))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_score_field.p, sqdist, bytes, hipMemcpyHostToDevice, h->stream));
        F.sqdist = (const int32_t *)h->d_score_field.p;
    }
    // with groups: the five words per ray of the whole batch, then the staging of a host group_begin and of a host table
    MlmClearGroups G{};
    char *g_words[5] = {};
    if (grouped) {
        const size_t N = (size_t)n, part[5] = {mlm_align256(N * sizeof(int64_t)), mlm_align256(N * sizeof(int32_t)), mlm_align256(N * sizeof(int32_t)),
                                               mlm_align256(N * sizeof(int32_t)), mlm_align256(N)};
        const size_t gb_bytes = gb_dev ? 0 : mlm_align256(((size_t)n_groups + 1) * sizeof(int32_t));
        const size_t tab_bytes = table_staged ? mlm_align256((size_t)n_groups * MLM_CLEAR_WORDS * sizeof(int64_t)) : 0;
        if ((rc = readout_reserve(h, h->d_clear, part[0] + part[1] + part[2] + part[3] + part[4] + gb_bytes + tab_bytes, "mlm_query_clearance"))) return rc;
        char *at = (char *)h->d_clear.p;
        for (int w = 0; w < 5; ++w) {
            g_words[w] = at;
            at += part[w];
        }
        G.begin = gb_dev ? group_begin : (const int32_t *)at;
        G.table = table_staged ? (int64_t *)(at + gb_bytes) : table;
        G.n_groups = n_groups;
        G.cost = (const int64_t *)g_words[0], G.min_sq = (const int32_t *)g_words[1], G.n_steps = (const int32_t *)g_words[2];
        G.n_near = (const int32_t *)g_words[3], G.status = (const int8_t *)g_words[4];
        if (!gb_dev) HIPCHK(h, hipMemcpyAsync(at, group_begin, ((size_t)n_groups + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
    // chunks: staged channels of a chunk share one kept buffer (at most 101 bytes per ray); one lane per ray, as k_rays
    void (*const kern)(const MlmClear) = h->clear_ahead == 4 ? k_clearance<4> : k_clearance<1>;
    if (n > 0) {
        const size_t chunk = (size_t)std::min(n, kClearChunk);
        if ((rc = ch.reserve(h, "mlm_query_clearance", chunk))) return rc;
        rc = chunk_rounds(h, ch, (size_t)n, chunk, 0, 2, 2, 10, [&](size_t i0, size_t m, void **at) {
            MlmClear R{(const double *)at[0], (const double *)at[1], (int)m, d, F, (int8_t *)at[2], (int32_t *)at[3], (double *)at[4], (int32_t *)at[5],
                       (int32_t *)at[6], (int32_t *)at[7], (int64_t *)at[8], (int32_t *)at[9], nullptr, nullptr, nullptr, nullptr, nullptr};
            if (grouped) {
                R.g_cost = (int64_t *)g_words[0] + i0, R.g_min_sq = (int32_t *)g_words[1] + i0, R.g_steps = (int32_t *)g_words[2] + i0;
                R.g_near = (int32_t *)g_words[3] + i0, R.g_status = (int8_t *)g_words[4] + i0;
            }
            launch(h, kern, lanes_grid(m, h->rays_grid), 0, R);
            return MLM_OK;
        });
        if (rc) return rc;
    }
    if (grouped && n_groups > 0) { // behind the last chunk: one lane per group
        launch(h, k_clearance_groups, lanes_grid((size_t)n_groups, kClearGroupGrid), 0, G);
        HIPCHK(h, hipGetLastError());
        if (table_staged)
            HIPCHK(h, hipMemcpyAsync(table, G.table, (size_t)n_groups * MLM_CLEAR_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

namespace {
constexpr int kViewChunkViews = 1 << 16;   // views per pass: bounds the job lists and the staged rows (64 bytes per view)
constexpr unsigned int kViewGrid = 1 << 16; // most workgroups of a launch (grid-stride over the jobs)
} // namespace

int mlm_query_views(mlm_handle *h, const double *p0, const double *p1, const int32_t *view_begin, int n_views, int flags, const int32_t lo[3],
                    const int32_t dims[3], const uint8_t *exclude, uint8_t *mark, int64_t *table) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const bool boxed = lo && dims;
    if (n_views < 0 || (n_views > 0 && !view_begin) || (flags & ~7) || (!mark && !table) || (!lo != !dims) || ((exclude || mark) && !boxed) ||
        (mark && mark == exclude)) {
        h->err = "mlm_query_views: negative n_views, a null view_begin, an unknown flag bit, no output, lo without dims, exclude or mark without "
                 "a box, or mark == exclude";
        return MLM_ERR_INVALID;
    }
    MlmViewWindow B{};
    long long D[3], nvox = 0;
    int rc;
    if (boxed) {
        B.on = 1;
        if ((rc = box_check(h, "mlm_query_views", lo, dims, D, nvox))) return rc;
        for (int a = 0; a < 3; ++a) {
            B.lo[a] = lo[a];
            B.d[a] = dims[a];
        }
    }
    if (n_views == 0) return MLM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // view_begin: validated on the host (copied back when it is device memory, behind the caller's work on the stream)
    std::vector<int32_t> vb_copy;
    const int32_t *vb = view_begin;
    if (readout_in_place(view_begin)) {
        vb_copy.resize((size_t)n_views + 1);
        HIPCHK(h, hipMemcpyAsync(vb_copy.data(), view_begin, vb_copy.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        vb = vb_copy.data();
    }
    bool vb_ok = vb[0] >= 0;
    for (int k = 0; k < n_views && vb_ok; ++k) vb_ok = vb[k + 1] >= vb[k];
    if (!vb_ok || (vb[n_views] > vb[0] && (!p0 || !p1))) {
        h->err = "mlm_query_views: view_begin must start at >= 0 and must not decrease; rays need p0 and p1";
        return MLM_ERR_INVALID;
    }
    if ((rc = drain(h))) return rc;

    long long lds_bits = kViewLdsBits, kv;
    if (knob("view_lds_bits", kv)) lds_bits = kv;
    const bool p_staged[2] = {p0 && !readout_in_place(p0), p1 && !readout_in_place(p1)};
    const bool ex_staged = exclude && !readout_in_place(exclude), mark_staged = mark && !readout_in_place(mark), table_staged = table && !readout_in_place(table);
    // a host exclude / mark: the whole box once (mark with its contents: bytes no view touches stay as they were)
    const size_t box_bytes = mlm_align256((size_t)nvox);
    if ((ex_staged || mark_staged) &&
        (rc = readout_reserve(h, h->d_win_stage, box_bytes * ((ex_staged ? 1 : 0) + (mark_staged ? 1 : 0)), "mlm_query_views")))
        return rc;
    const uint8_t *d_exclude = exclude;
    uint8_t *d_mark = mark;
    if (ex_staged) {
        d_exclude = (const uint8_t *)h->d_win_stage.p;
        HIPCHK(h, hipMemcpyAsync(h->d_win_stage.p, exclude, (size_t)nvox, hipMemcpyHostToDevice, h->stream));
    }
    if (mark_staged) {
        d_mark = (uint8_t *)h->d_win_stage.p + (ex_staged ? box_bytes : 0);
        HIPCHK(h, hipMemcpyAsync(d_mark, mark, (size_t)nvox, hipMemcpyHostToDevice, h->stream));
    }

    std::vector<long long> begin;
    std::vector<MlmViewJob> jobs;
    std::vector<MlmViewBox> raw;
    for (int k0 = 0; k0 < n_views;) {
        // a chunk of views: at most kViewChunkViews, and with staged rays at most kRayChunk rays (a longer view on its own)
        int k1 = k0 + 1;
        while (k1 < n_views && k1 - k0 < kViewChunkViews && (!(p_staged[0] || p_staged[1]) || (long long)vb[k1 + 1] - vb[k0] <= kRayChunk)) ++k1;
        const int nv = k1 - k0;
        const long long r0 = vb[k0], nr = (long long)vb[k1] - r0;
        begin.resize((size_t)nv + 1);
        for (int k = 0; k <= nv; ++k) begin[(size_t)k] = (long long)vb[k0 + k] - r0;
        const double *ray[2] = {p0, p1};
        const size_t ray_bytes = mlm_align256((size_t)nr * 3 * sizeof(double));
        if (nr && (p_staged[0] || p_staged[1]) &&
            (rc = readout_reserve(h, h->d_ray_stage, ray_bytes * ((p_staged[0] ? 1 : 0) + (p_staged[1] ? 1 : 0)), "mlm_query_views")))
            return rc;
        for (int c = 0; c < 2; ++c) {
            if (!nr) continue;
            if (p_staged[c]) {
                double *at = (double *)((char *)h->d_ray_stage.p + (c && p_staged[0] ? ray_bytes : 0));
                HIPCHK(h, hipMemcpyAsync(at, ray[c] + 3 * (size_t)r0, (size_t)nr * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
                ray[c] = at;
            } else {
                ray[c] += 3 * (size_t)r0;
            }
        }
        // the views' bounding boxes
        jobs.clear();
        for (int k = 0; k < nv; ++k)
            for (long long i = begin[(size_t)k]; i < begin[(size_t)k + 1]; i += kViewBoxRays)
                jobs.push_back(MlmViewJob{k, (int)i, (int)std::min(i + kViewBoxRays, begin[(size_t)k + 1]), 0, 1, 0, 0});
        const size_t raw_bytes = mlm_align256((size_t)nv * sizeof(MlmViewBox));
        if ((rc = readout_reserve(h, h->d_views, raw_bytes + mlm_align256(jobs.size() * sizeof(MlmViewJob)), "mlm_query_views"))) return rc;
        MlmViewBox *d_raw = (MlmViewBox *)h->d_views.p;
        MlmViewJob *d_jobs = (MlmViewJob *)((char *)h->d_views.p + raw_bytes);
        hipLaunchKernelGGL(k_views_box_init, dim3((unsigned int)((nv + 255) / 256)), dim3(256), 0, h->stream, d_raw, nv);
        if (!jobs.empty()) {
            HIPCHK(h, hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(MlmViewJob), hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_views_box, dim3((unsigned int)std::min<size_t>(jobs.size(), kViewGrid)), dim3(256), 0, h->stream, h->P, ray[0], ray[1],
                               (const MlmViewJob *)d_jobs, (int)jobs.size(), d_raw);
        }
        HIPCHK(h, hipGetLastError());
        raw.resize((size_t)nv);
        HIPCHK(h, hipMemcpyAsync(raw.data(), d_raw, (size_t)nv * sizeof(MlmViewBox), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        // the plan, its lists and the scratch (the kept buffer may move: the boxes go up again)
        const MlmViewPlan plan = mlm_view_plan(raw.data(), begin.data(), nv, B, lds_bits);
        jobs.clear();
        size_t first[kViewLdsClasses + 1];
        for (int c = 0; c < kViewLdsClasses; ++c) {
            first[c] = jobs.size();
            jobs.insert(jobs.end(), plan.lds[c].begin(), plan.lds[c].end());
        }
        first[kViewGlobal] = jobs.size();
        jobs.insert(jobs.end(), plan.global.begin(), plan.global.end());
        const size_t jobs_bytes = mlm_align256(jobs.size() * sizeof(MlmViewJob)), ref_bytes = mlm_align256(plan.refused.size() * sizeof(int)),
                     rows_bytes = table_staged ? mlm_align256((size_t)nv * kViewRow * sizeof(int64_t)) : 0;
        if ((rc = readout_reserve(h, h->d_views, raw_bytes + jobs_bytes + ref_bytes + rows_bytes + (size_t)plan.scratch_words * 4, "mlm_query_views")))
            return rc;
        char *base = (char *)h->d_views.p;
        d_raw = (MlmViewBox *)base;
        d_jobs = (MlmViewJob *)(base + raw_bytes);
        int *d_ref = (int *)(base + raw_bytes + jobs_bytes);
        int64_t *rows = !table ? nullptr : table_staged ? (int64_t *)(base + raw_bytes + jobs_bytes + ref_bytes) : table + (size_t)k0 * kViewRow;
        HIPCHK(h, hipMemcpyAsync(d_raw, raw.data(), (size_t)nv * sizeof(MlmViewBox), hipMemcpyHostToDevice, h->stream));
        if (!jobs.empty()) HIPCHK(h, hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(MlmViewJob), hipMemcpyHostToDevice, h->stream));
        if (rows) HIPCHK(h, hipMemsetAsync(rows, 0, (size_t)nv * kViewRow * sizeof(int64_t), h->stream));
        MlmViews V{ray[0], ray[1], flags, B, d_exclude, d_mark, d_raw, rows, (uint32_t *)(base + raw_bytes + jobs_bytes + ref_bytes + rows_bytes)};
        for (int c = 0; c < kViewLdsClasses; ++c) {
            const size_t nj = first[c + 1] - first[c];
            if (!nj) continue;
            hipLaunchKernelGGL(k_views_lds, dim3((unsigned int)std::min<size_t>(nj, kViewGrid)), dim3(kViewLdsThreads), (size_t)mlm_view_class_bytes(c),
                               h->stream, h->P, V, (const MlmViewJob *)(d_jobs + first[c]), (int)nj);
        }
        HIPCHK(h, hipGetLastError());
        for (const MlmViewPlan::Batch &b : plan.batches) {
            HIPCHK(h, hipMemsetAsync(V.scratch, 0, (size_t)b.words * 4, h->stream));
            const size_t nj = b.job1 - b.job0;
            hipLaunchKernelGGL(k_views_global, dim3((unsigned int)std::min<size_t>(nj, kViewGrid)), dim3(kViewGlobalThreads), 0, h->stream, h->P, V,
                               (const MlmViewJob *)(d_jobs + first[kViewGlobal] + b.job0), (int)nj);
            HIPCHK(h, hipGetLastError());
        }
        if (rows && !plan.refused.empty()) {
            HIPCHK(h, hipMemcpyAsync(d_ref, plan.refused.data(), plan.refused.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_views_refused, dim3((unsigned int)((plan.refused.size() + 255) / 256)), dim3(256), 0, h->stream, rows,
                               (const int *)d_ref, (int)plan.refused.size());
            HIPCHK(h, hipGetLastError());
        }
        if (table_staged)
            HIPCHK(h, hipMemcpyAsync(table + (size_t)k0 * kViewRow, rows, (size_t)nv * kViewRow * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream)); // (the lists above are reused by the next chunk)
        k0 = k1;
    }
    if (mark_staged) {
        HIPCHK(h, hipMemcpyAsync(mark, d_mark, (size_t)nvox, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return MLM_OK;
}

int mlm_export_block_flags(mlm_handle *h, int cap, uint8_t *collapsed, int *n_out) {
    if (!h || cap < 0) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    int n = 0;
    int rc = mlm_block_count(h, &n);
    if (rc) return rc;
    if (n_out) *n_out = n;
    const size_t m = (size_t)std::min(n, cap);
    if (!m || !collapsed) return MLM_OK;
    if (h->P.explore)
        HIPCHK(h, hipMemcpy(collapsed, h->P.blk_collapsed, m, hipMemcpyDefault));
    else
        std::memset(collapsed, 0, m);
    return MLM_OK;
}

int mlm_export_frontier(mlm_handle *h, int cap, int32_t *keys_cell, int *n_out) {
    if (!h || cap < 0 || (cap > 0 && !keys_cell)) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (n_out) *n_out = 0;
    if (!h->P.explore) return MLM_OK;
    int nb = 0;
    int rc = mlm_block_count(h, &nb);
    if (rc) return rc;
    int32_t *d_out = nullptr;
    unsigned int *d_cnt = nullptr;
    HIPCHK(h, hipMalloc((void **)&d_out, std::max<size_t>((size_t)cap * 4 * sizeof(int32_t), 16)));
    HIPCHK(h, hipMalloc((void **)&d_cnt, sizeof(unsigned int)));
    HIPCHK(h, hipMemsetAsync(d_cnt, 0, sizeof(unsigned int), h->stream));
    if (nb > 0)
        launch(h, k_ex_export_frontier, 512u, 0, h->P, (unsigned int)nb, d_out, (unsigned int)cap, d_cnt);
    unsigned int cnt = 0;
    hipError_t e = hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && cnt && cap)
        e = hipMemcpy(keys_cell, d_out, (size_t)std::min<unsigned int>(cnt, (unsigned int)cap) * 4 * sizeof(int32_t), hipMemcpyDefault);
    hipFree(d_out);
    hipFree(d_cnt);
    if (e != hipSuccess) {
        h->err = std::string("mlm_export_frontier: ") + hipGetErrorString(e);
        return MLM_ERR_HIP;
    }
    if (n_out) *n_out = (int)cnt;
    return MLM_OK;
}

static int export_points(mlm_handle *h, int cap_points, float *xyz, int *n_out, int which, const char *what) {
    HIPCHK(h, hipSetDevice(h->device));
    if (n_out) *n_out = 0;
    if (which == 1 && !h->P.explore) return MLM_OK; // frontier sets only exist with use_exploration_frontiers
    int nb = 0;
    int rc = mlm_block_count(h, &nb);
    if (rc) return rc;
    float *d_xyz = nullptr;
    unsigned int *d_cnt = nullptr;
    HIPCHK(h, hipMalloc((void **)&d_xyz, std::max<size_t>((size_t)cap_points * 3 * sizeof(float), 16)));
    hipError_t e = hipMalloc((void **)&d_cnt, sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, sizeof(unsigned int), h->stream);
    if (e == hipSuccess && nb > 0)
        launch(h, k_export_global, 1024u, 0, h->P, (unsigned int)nb, d_xyz, (unsigned int)cap_points, d_cnt, which);
    unsigned int cnt = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && cnt && cap_points)
        e = hipMemcpy(xyz, d_xyz, (size_t)std::min<unsigned int>(cnt, (unsigned int)cap_points) * 3 * sizeof(float),
                      hipMemcpyDefault);
    hipFree(d_xyz);
    if (d_cnt) hipFree(d_cnt);
    if (e != hipSuccess) {
        h->err = std::string(what) + ": " + hipGetErrorString(e);
        return MLM_ERR_HIP;
    }
    if (n_out) *n_out = (int)cnt;
    return MLM_OK;
}

int mlm_export_global_map(mlm_handle *h, int cap_points, float *xyz, int *n_out) {
    if (!h || cap_points < 0 || (cap_points > 0 && !xyz)) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    return export_points(h, cap_points, xyz, n_out, 0, "mlm_export_global_map");
}

int mlm_export_frontier_points(mlm_handle *h, int cap_points, float *xyz, int *n_out) {
    if (!h || cap_points < 0 || (cap_points > 0 && !xyz)) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    return export_points(h, cap_points, xyz, n_out, 1, "mlm_export_frontier_points");
}

namespace {
// the one staging buffer of an import of N blocks: keys | slots | log_odds | occ | infl | collapsed
struct ImportStage {
    size_t o_keys, o_slots, o_lo, o_occ, o_infl, o_col, total;
};
ImportStage import_stage(size_t N, size_t C) {
    ImportStage L{};
    L.o_keys = 0, L.o_slots = L.o_keys + N * 12, L.o_lo = (L.o_slots + N * 4 + 15) & ~(size_t)15, L.o_occ = L.o_lo + N * C * 4, L.o_infl = L.o_occ + N * C,
    L.o_col = L.o_infl + N * C, L.total = L.o_col + N;
    return L;
}
// The n blocks staged at d (device memory; a plane that is not staged is left as it is in the map) found or created and overwritten;
// waits, and reports a pool that could not take them.  mlm_import_blocks, and the last step of mlm_warp_blocks' MLM_WARP_REPLACE.
int import_staged(mlm_handle *h, char *d, const ImportStage &L, int n, bool log_odds, bool occ, bool infl, bool collapsed) {
    const size_t C = (size_t)h->P.cells, N = (size_t)n;
    launch(h, k_import_slots, grid_for(N), 0, h->P, (const int32_t *)(d + L.o_keys), n, (int *)(d + L.o_slots));
    launch(h, k_import_cells, lanes_grid(N * C, 4096u), 0, h->P, (const int *)(d + L.o_slots), n, log_odds ? (const float *)(d + L.o_lo) : nullptr,
           occ ? (const uint8_t *)(d + L.o_occ) : nullptr, infl ? (const uint8_t *)(d + L.o_infl) : nullptr,
           collapsed ? (const uint8_t *)(d + L.o_col) : nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->err = std::string("mlm_import_blocks: ") + hipGetErrorString(e);
        return MLM_ERR_HIP;
    }
    const int rc = read_global(h);
    if (rc) return rc;
    if (h->h_g->err) {
        h->err = "block pool or block hash table full (raise mlm_limits.max_blocks)";
        clear_device_error(h);
        return MLM_ERR_CAPACITY;
    }
    return MLM_OK;
}
} // namespace

int mlm_import_blocks(mlm_handle *h, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl,
                      const uint8_t *collapsed) {
    if (!h || n < 0 || (n > 0 && !keys)) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc || n == 0) return rc;
    mirror_mark_all(h);
    rc = ensure_free_blocks_idle(h, (size_t)n);
    if (rc) return rc;
    const size_t C = (size_t)h->P.cells, N = (size_t)n;
    // (sources may be host or device memory)
    const ImportStage L = import_stage(N, C);
    char *d = nullptr;
    HIPCHK(h, hipMalloc((void **)&d, L.total));
    DevTmp stage{d};
    hipError_t e = hipMemcpyAsync(d + L.o_keys, keys, N * 12, hipMemcpyDefault, h->stream);
    if (e == hipSuccess && log_odds) e = hipMemcpyAsync(d + L.o_lo, log_odds, N * C * 4, hipMemcpyDefault, h->stream);
    if (e == hipSuccess && occ) e = hipMemcpyAsync(d + L.o_occ, occ, N * C, hipMemcpyDefault, h->stream);
    if (e == hipSuccess && infl) e = hipMemcpyAsync(d + L.o_infl, infl, N * C, hipMemcpyDefault, h->stream);
    if (e == hipSuccess && collapsed) e = hipMemcpyAsync(d + L.o_col, collapsed, N, hipMemcpyDefault, h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        h->err = std::string("mlm_import_blocks: ") + hipGetErrorString(e);
        return MLM_ERR_HIP;
    }
    return import_staged(h, d, L, n, log_odds != nullptr, occ != nullptr, infl != nullptr, collapsed != nullptr);
}

namespace {
static_assert(MLM_CROP_INSIDE == MLM_CROP_F_INSIDE && MLM_CROP_DRY == MLM_CROP_F_DRY && MLM_CROP_SHRINK == MLM_CROP_F_SHRINK && MLM_CROP_OUTSIDE == 0,
              "mlm_crop.h restates the flags of include/mlmap_hip.h");
constexpr unsigned int kCropGrid = 8192; // most workgroups of the crop kernels (they stride over the rest)

// the copy kernel K<FW, BW> for the lane widths fw (16 or 4 bytes: float plane) and bw (16, 4 or 1 bytes: byte planes)
#define MLM_CROP_LAUNCH(K, fw, bw, grid, ...)                                                                                     \
    do {                                                                                                                          \
        if ((fw) == 16 && (bw) == 16) hipLaunchKernelGGL((K<16, 16>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);    \
        else if ((fw) == 16 && (bw) == 4) hipLaunchKernelGGL((K<16, 4>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__); \
        else if ((fw) == 16) hipLaunchKernelGGL((K<16, 1>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);              \
        else if ((bw) == 16) hipLaunchKernelGGL((K<4, 16>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);              \
        else if ((bw) == 4) hipLaunchKernelGGL((K<4, 4>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);                \
        else hipLaunchKernelGGL((K<4, 1>), dim3(grid), dim3(MLM_BLOCK), 0, h->stream, __VA_ARGS__);                               \
    } while (0)
inline int crop_width(int w, const void *p) { // the widest lane path of at most w bytes that p's alignment allows
    const uintptr_t a = (uintptr_t)p;
    return !p ? w : (w >= 16 && a % 16 == 0) ? 16 : (w >= 4 && a % 4 == 0) ? 4 : 1;
}

// The slots [K, nb) back at alloc_pool's initial values, on the handle's stream (a null-stream hipMemset is not ordered with it: grow_pool).
int crop_reset_tail(mlm_handle *h, unsigned int K, unsigned int nb) {
    const MlmDev &P = h->P;
    const size_t C = (size_t)P.cells, v0 = (size_t)K * C, nv = (size_t)(nb - K) * C;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemsetAsync(P.log_odds + v0, 0, nv * sizeof(float), st));
    HIPCHK(h, hipMemsetAsync(P.occ + v0, 'u', nv, st));
    HIPCHK(h, hipMemsetAsync(P.infl + v0, 'u', nv, st));
    for (int half = 0; half < 2; ++half) {
        HIPCHK(h, hipMemsetAsync(P.vox_head + half * P.vox_stride + v0, 0xFF, nv * sizeof(int), st));
        HIPCHK(h, hipMemsetAsync(P.vox_miss + half * P.vox_stride + v0, 0, nv * sizeof(uint32_t), st));
    }
    if (P.explore) {
        HIPCHK(h, hipMemsetAsync(P.frnt + v0, 0, nv, st));
        HIPCHK(h, hipMemsetAsync(P.vox_tau + v0, 0, nv * sizeof(unsigned long long), st));
        HIPCHK(h, hipMemsetAsync(P.blk_collapsed + K, 0, (size_t)(nb - K), st));
        HIPCHK(h, hipMemsetAsync(P.blk_observed + K, 0, (size_t)(nb - K), st));
    }
    return MLM_OK;
}

// The tail of a call that drops blocks (mlm_crop_blocks, mlm_age_blocks with MLM_AGE_DROP), behind every check, count and allocation:
// `list` is mlm_crop.h's list over the nb slots in use — the D dropped ones in front — and H the pairs of the move.  The pool is
// compacted by hole filling, the free tail reset, the table rebuilt, the block count set on both sides; g is the global state afterwards.
int crop_compact(mlm_handle *h, const unsigned int *list, unsigned int nb, unsigned int D, unsigned int K, unsigned int H, MlmGlobal &g) {
    int rc;
    const int fw = mlm_crop_float_width(h->P.cells), bw = mlm_crop_byte_width(h->P.cells);
    // From here on the pool changes.  The host mirror maps pool slot s to its own slot s: it forgets which blocks it knows.
    mirror_finish_eager(h);
    if (h->mir.cap) h->mir.view.table_reset(h->mir.cap);
    h->mir.n_known = 0;
    mirror_mark_all(h);
    if (H) {
        MLM_CROP_LAUNCH(k_crop_move, fw, bw, wave_grid(H, kCropGrid), h->P, list, nb, D, K, H);
        HIPCHK(h, hipGetLastError());
    }
    if ((rc = crop_reset_tail(h, K, nb))) return rc;
    const size_t ht = (size_t)h->P.ht_mask + 1;
    HIPCHK(h, hipMemsetAsync(h->P.ht_keys, 0xFF, ht * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(h->P.ht_slot, 0xFF, ht * sizeof(int), h->stream));
    if (K) {
        launch(h, k_rehash_blocks, grid_for(K), 0, h->P, K);
        HIPCHK(h, hipGetLastError());
    }
    g = *h->h_g;
    g.n_blocks = K;
    g.err &= ~1u;
    HIPCHK(h, hipMemcpyAsync(h->P.g, &g, sizeof(g), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *h->h_g = g;
    for (int k = 0; k < MLM_SETS; ++k) *h->h_gb[k] = g;
    h->stats.n_blocks = K;
    return MLM_OK;
}

// everything of mlm_crop_blocks behind the argument check and the drain
int crop_run(mlm_handle *h, const MlmCropBox &B, int flags, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl,
             uint8_t *collapsed, int64_t *summary) {
    int64_t sum[MLM_CROP_ROW] = {};
    auto report = [&]() {
        sum[7] = (int64_t)h->alloc_bytes;
        if (summary) std::memcpy(summary, sum, sizeof(sum));
    };
    int rc = read_global(h);
    if (rc) return rc;
    const unsigned int nb = std::min<unsigned int>(h->h_g->n_blocks, (unsigned int)h->P.max_blocks);
    h->stats.n_blocks = nb; // (mlm_frame_stats follows the calls that change the block count between frames as well)
    h->stats.block_capacity = h->P.max_blocks;
    sum[0] = sum[1] = nb;
    sum[4] = sum[5] = h->P.max_blocks;
    sum[6] = sum[7] = (int64_t)h->alloc_bytes;
    const bool any_out = keys || log_odds || occ || infl || collapsed;
    unsigned int D = 0, H = 0;
    const unsigned int chunks = (nb + MLM_CROP_SLOTS_PER_CHUNK - 1) / MLM_CROP_SLOTS_PER_CHUNK;
    unsigned int *chunk_cnt = nullptr, *ctrl = nullptr, *list = nullptr;
    if (nb) {
        // chunk counts | ctrl | list: 4 bytes per block, kept by the handle as the read-outs keep theirs
        const size_t o_ctrl = mlm_align256((size_t)chunks * 4), o_list = o_ctrl + 256, total = o_list + (size_t)nb * 4;
        if ((rc = readout_reserve(h, h->d_crop, total, "mlm_crop_blocks"))) {
            report();
            return rc;
        }
        void *scratch = h->d_crop.p;
        chunk_cnt = (unsigned int *)scratch, ctrl = (unsigned int *)((char *)scratch + o_ctrl), list = (unsigned int *)((char *)scratch + o_list);
        const unsigned int grid = std::min(chunks, kCropGrid);
        HIPCHK(h, hipMemsetAsync(ctrl, 0, MLM_CROP_CTRL_WORDS * 4, h->stream));
        launch(h, k_crop_count, grid, 0, h->P, B, nb, chunks, chunk_cnt);
        launch(h, k_crop_scan, 1u, 0, chunk_cnt, chunks, ctrl);
        launch(h, k_crop_list, grid, 0, h->P, B, nb, chunks, chunk_cnt, ctrl, list);
        HIPCHK(h, hipGetLastError());
        const unsigned int *c;
        if ((rc = read_back(h, (const unsigned int *)ctrl, MLM_CROP_CTRL_WORDS, c))) return rc;
        D = c[0], H = c[1];
        if (D > nb || H > std::min(D, nb - D)) {
            h->err = "mlm_crop_blocks: the scan of the drop flags is inconsistent";
            return MLM_ERR_HIP;
        }
    }
    const unsigned int K = nb - D;
    sum[1] = K, sum[2] = D;
    if (any_out && (unsigned int)cap < D) {
        h->err = "mlm_crop_blocks: " + std::to_string(D) + " blocks would be dropped, the outputs hold " + std::to_string(cap);
        report();
        return MLM_ERR_CAPACITY;
    }
    if ((flags & MLM_CROP_DRY) || D == 0) {
        report();
        return MLM_OK;
    }
    const size_t C = (size_t)h->P.cells;
    const int fw = mlm_crop_float_width(h->P.cells), bw = mlm_crop_byte_width(h->P.cells);
    if (any_out) { // the page-out first: the holes are among its sources
        ReadoutChannels<5> ch(h->d_win_stage, {{keys, 3 * sizeof(int32_t)}, {log_odds, C * sizeof(float)}, {occ, C}, {infl, C}, {collapsed, 1}});
        const size_t rows = page_rows(ch, D);
        if ((rc = ch.reserve(h, "mlm_crop_blocks", rows))) {
            report();
            return rc;
        }
        rc = page_rounds(h, ch, D, rows, [&](size_t r0, size_t r1) {
            float *d_lo = (float *)ch.at(1, r0);
            uint8_t *d_occ = (uint8_t *)ch.at(2, r0), *d_infl = (uint8_t *)ch.at(3, r0);
            const int pfw = crop_width(fw, d_lo), pbw = std::min(crop_width(bw, d_occ), crop_width(bw, d_infl));
            MLM_CROP_LAUNCH(k_crop_page, pfw, pbw, wave_grid(r1 - r0, kCropGrid), h->P, (const unsigned int *)list, nb, (unsigned int)r0, (unsigned int)r1,
                            (int32_t *)ch.at(0, r0), d_lo, d_occ, d_infl, (uint8_t *)ch.at(4, r0));
        });
        if (rc) return rc;
        sum[3] = D;
    }
    MlmGlobal g{};
    if ((rc = crop_compact(h, (const unsigned int *)list, nb, D, K, H, g))) return rc;
    if ((flags & MLM_CROP_SHRINK) && h->pool_grow) { // best effort: the crop stands whether or not the smaller pool could be had
        const long long target = mlm_crop_shrink_target(h->lim.max_blocks, h->P.max_blocks, K);
        if (target > 0) {
            const std::string err = h->err;
            rc = resize_pool(h, (size_t)target, g, K);
            if (rc == MLM_ERR_CAPACITY) {
                h->err = err;
            } else if (rc) {
                return rc;
            } else {
                h->grow_failed_at = 0; // (memory went back to the device: what did not fit before may fit now)
                if (getenv("MLM_DEBUG_CREATE")) fprintf(stderr, "[pool] shrunk to %d blocks (%u in use)\n", h->P.max_blocks, K);
            }
        }
    }
    h->stats.block_capacity = h->P.max_blocks;
    sum[5] = h->P.max_blocks;
    sum[7] = (int64_t)h->alloc_bytes;
    report();
    return MLM_OK;
}
} // namespace

int mlm_crop_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int flags, int cap, int32_t *keys, float *log_odds,
                    uint8_t *occ, uint8_t *infl, uint8_t *collapsed, int64_t summary[MLM_CROP_ROW]) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    MlmCropBox B{};
    if (const int bad = mlm_crop_check(key_lo, key_dims, flags, cap, B)) {
        h->err = std::string("mlm_crop_blocks: ") + mlm_crop_check_text(bad);
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc) return rc;
    return crop_run(h, B, flags, cap, keys, log_odds, occ, infl, collapsed, summary);
}

#include "mlm_warp_host.h"
#include "mlm_fuse_host.h"
#include "mlm_age_host.h"
#include "mlm_delta_host.h"
#include "mlm_pack_host.h"

int mlm_merge_pack(mlm_handle *h, const int32_t *keys_dev, int n, float *log_odds_dev, uint8_t *seen_dev) {
    if (!h || n < 0 || (n > 0 && (!keys_dev || !log_odds_dev || !seen_dev))) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    if (rc || n == 0) return rc;
    launch(h, k_merge_pack, lanes_grid((size_t)n * h->P.cells, 8192u), 0, h->P, keys_dev, n, log_odds_dev, seen_dev);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_merge_finish(mlm_handle *h, float *log_odds_dev, const uint8_t *seen_dev, size_t n_cells, uint8_t *occ_dev) {
    if (!h || (n_cells > 0 && (!log_odds_dev || !seen_dev || !occ_dev))) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    if (n_cells == 0) return MLM_OK;
    launch(h, k_merge_finish, lanes_grid(n_cells, 8192u), 0, h->P, log_odds_dev, seen_dev, n_cells, occ_dev);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_query_odds_at(mlm_handle *h, const int32_t *glb_id, const int32_t *subbox_id, int n, float *out) {
    if (!h || !glb_id || !subbox_id || !out || n < 0) return MLM_ERR_INVALID;
    for (int i = 0; i < n; ++i) // std::vector::operator[] out of range is undefined behaviour in the reference
        if (subbox_id[i] < 0 || subbox_id[i] >= h->P.cells) return MLM_ERR_INVALID;
    if (n == 0) return MLM_OK;
    MLM_LOCK(h);
    if (mirror_wanted(h, 3, n, 0)) { // (mlm_mirror.h)
        const int rc = mirror_sync(h);
        if (rc == MLM_OK) {
            for (int i = 0; i < n; ++i) out[i] = mir_odd_at(h, glb_id[3 * (size_t)i], glb_id[3 * (size_t)i + 1], glb_id[3 * (size_t)i + 2], subbox_id[i]);
            h->mir.n_host_queries += n;
            return MLM_OK;
        }
        if (!h->mir.alloc_failed && rc != kMirrorUnavailable) return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain(h);
    if (rc) return rc;
    rc = ensure_query(h, (size_t)n);
    if (rc) return rc;
    int32_t *d_g = (int32_t *)h->d_qpos, *d_s = d_g + 3 * (size_t)n;
    HIPCHK(h, hipMemcpyAsync(d_g, glb_id, (size_t)n * 12, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_s, subbox_id, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    launch(h, k_query_odds_at, grid_for((size_t)n), 0, h->P, d_g, d_s, n, (float *)h->d_qout);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_qout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MLM_OK;
}

int mlm_sync(mlm_handle *h) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    return drain(h);
}

int mlm_set_async(mlm_handle *h, int on) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    h->async_mode = on != 0;
    return rc;
}

int mlm_set_host_mirror_limit(mlm_handle *h, size_t max_bytes) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    h->mir.max_bytes = max_bytes;
    HIPCHK(h, hipSetDevice(h->device));
    mirror_apply_limit(h); // (mlm_mirror.h)
    return MLM_OK;
}

int mlm_get_frame_stats(mlm_handle *h, mlm_frame_stats *out) {
    if (!h || !out) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    *out = h->stats;
    out->n_host_queries = h->mir.n_host_queries;
    out->n_mirror_refreshes = h->mir.n_refresh;
    out->n_mirror_blocks = h->mir.n_copied;
    out->device_bytes = (int64_t)h->alloc_bytes;
    out->n_slot_grows = h->n_slot_grows;
    return MLM_OK;
}

int mlm_get_awareness_hits(mlm_handle *h, int cap, uint32_t *cell_idx, float *odds, uint32_t *t_first, int *n_out) {
    if (!h || cap < 0) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    {
        const int rc = drain(h);
        if (rc) return rc;
    }
    if (odds && !h->P.record_awareness && !h->P.explore) { // (the kernels keep the odds themselves only for this read-back)
        h->err = "mlm_limits.record_awareness was not set";
        return MLM_ERR_INVALID;
    }
    const MlmDev &P = eff_params(h, h->slots[(size_t)h->last_slot]);
    const size_t n = (size_t)h->stats.n_hit_cells;
    if (n_out) *n_out = (int)n;
    const size_t m = std::min<size_t>(n, (size_t)cap);
    if (m == 0) return MLM_OK;
    if (cell_idx) HIPCHK(h, hipMemcpy(cell_idx, P.hl_cell, m * 4, hipMemcpyDeviceToHost));
    if (odds) HIPCHK(h, hipMemcpy(odds, P.hl_odd, m * 4, hipMemcpyDeviceToHost));
    if (t_first) HIPCHK(h, hipMemcpy(t_first, P.hl_t, m * 4, hipMemcpyDeviceToHost));
    return MLM_OK;
}

int mlm_get_awareness_misses(mlm_handle *h, int cap, uint32_t *cell_idx, int *n_out) {
    if (!h || cap < 0) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    if (!h->P.record_awareness && !h->P.explore) {
        h->err = "mlm_limits.record_awareness was not set";
        return MLM_ERR_INVALID;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const MlmDev &P = h->slots[(size_t)h->last_slot].P;
    const size_t n = (size_t)h->stats.n_miss_cells;
    if (n_out) *n_out = (int)n;
    const size_t m = std::min<size_t>(n, (size_t)cap);
    if (m && cell_idx) HIPCHK(h, hipMemcpy(cell_idx, P.explore ? P.ex_cell : P.ml_cell, m * 4, hipMemcpyDeviceToHost));
    return MLM_OK;
}

int mlm_get_T_ls(mlm_handle *h, double q[4], double t[3]) {
    if (!h || !q || !t) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    const MlmFrame &F = h->slots[(size_t)h->last_slot].F;
    for (int i = 0; i < 4; ++i) q[i] = F.q_ls[i];
    for (int i = 0; i < 3; ++i) t[i] = F.t_ls[i];
    return MLM_OK;
}

int mlm_get_odds_table(mlm_handle *h, float *out) {
    if (!h || !out) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    std::memcpy(out, h->odds_table.data(), h->odds_table.size() * sizeof(float));
    return MLM_OK;
}

int mlm_enable_kernel_timing(mlm_handle *h, int on) {
    if (!h) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = drain(h);
    h->timing = on;
    h->ktimes.clear();
    h->kpool_used = 0;
    return rc;
}

int mlm_set_timed_kernel(mlm_handle *h, const char *name, int every) {
    if (!h || !name || every < 1) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    h->timed_kernel = name;
    h->timed_every = (unsigned int)every;
    h->timed_count = 0;
    return MLM_OK;
}

int mlm_get_kernel_times(mlm_handle *h, int cap, const char **names, float *ms, int *n_out) {
    if (!h || cap < 0) return MLM_ERR_INVALID;
    MLM_LOCK(h);
    HIPCHK(h, hipSetDevice(h->device));
    {
        const int rc = drain(h);
        if (rc) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    const int n = (int)h->ktimes.size();
    if (n_out) *n_out = n;
    for (int i = 0; i < std::min(n, cap); ++i) {
        float t = 0.f;
        hipEventElapsedTime(&t, h->ktimes[i].a, h->ktimes[i].b);
        if (names) names[i] = h->ktimes[i].name;
        if (ms) ms[i] = t;
    }
    if (h->timing >= 2 && cap >= n) { // accumulate modes: reading the list consumes it
        h->ktimes.clear();
        h->kpool_used = 0;
    }
    return MLM_OK;
}

} // extern "C"

#ifdef MLM_PHASE_PROF
// diagnostic build only: the same for k_tile (thread 0's clock per phase, summed over tiles and launches; cleared)
extern "C" int mlm_debug_tile_phases(unsigned long long *out8) {
    hipDeviceSynchronize();
    std::vector<unsigned long long> v((size_t)4096 * 8);
    if (hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(g_mlm_tphase), v.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
    for (int k = 0; k < 8; ++k) out8[k] = 0;
    for (size_t i = 0; i < v.size(); ++i) out8[i & 7] += v[i];
    std::fill(v.begin(), v.end(), 0ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_mlm_tphase), v.data(), v.size() * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
// diagnostic build only: workgroup spans of k_sector [0..3] and k_tile [4..7] — first start, last end, longest workgroup (10 ns
// ticks), workgroups — since the last call (cleared)
extern "C" int mlm_debug_spans(unsigned long long *out32) {
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_mlm_span), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[32];
    for (int k = 0; k < 32; ++k) z[k] = (k & 3) == 0 ? ~0ull : 0ull;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_mlm_span), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
extern "C" int mlm_debug_wg_times(unsigned long long *out) { // [2][2048][2]
    hipDeviceSynchronize();
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mlm_wg), 2 * 2048 * 2 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
// diagnostic build only: sum over blocks and clear the per-phase cycle counts of k_bin_points
extern "C" int mlm_debug_phases(unsigned long long *out16) {
    hipDeviceSynchronize();
    std::vector<unsigned long long> v((size_t)MLM_PHASE_BLOCKS * 16);
    if (hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(g_mlm_phase), v.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
    for (int k = 0; k < 16; ++k) out16[k] = 0;
    for (size_t i = 0; i < v.size(); ++i) out16[i & 15] += v[i];
    std::fill(v.begin(), v.end(), 0ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_mlm_phase), v.data(), v.size() * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
