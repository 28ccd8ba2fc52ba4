// mlm_plan.h — everything mlm_create decides WITHOUT the device, as one pure function: the constants of MlmDev, the LDS sizes and
// launch geometries of the kernels, the tile edge, the envelope that puts a configuration on the sector path or the cell-table path,
// the host tables and the capacities of the frame slots, from mlm_config, mlm_limits, the knobs and the device's CU count.  Plain
// C++17, no HIP: tests/test_create_plan.py builds it with g++ -fsanitize=address,undefined (tests/cpp/create_plan_driver.cpp) and holds
// it to tests/golden/create_plan.json.  mlm_create (mlmap_hip.hip) copies the plan into the handle and runs the device stages of
// mlm_resources.h with it.
#pragma once
#include <string>

#include "../../include/mlmap_hip.h"
#include "mlm_host.h"

#ifndef MLM_SETS
#define MLM_SETS 3
#endif
// MLM_SETS slot sets: batches in flight (one being filled, one in Stage A, one draining).  Measured on config 2 with the sector
// path: round 2 44.7k frames/s with 2, 48.4k with 3, 45.3k with 4; round 3 74.0k / 80.9k / 78.7k

constexpr int kRenderTileDefault = 2;        // k_render's tile: 0 64 x 1, 1 16 x 4, 2 8 x 8 (profiles/render_rate.json)

// capacities of a frame slot's lists that are sized by need (mlm_handle::need_sized)
struct MlmSlotCaps {
    size_t hl = 0, mt = 0, vh = 0, rec = 0, refs = 0, sub = 0, sbkt = 0;
};
// the limits of the host mirror (MlmMirror, mlm_handle.h)
struct MlmMirrorLimits {
    bool enabled = true;           // knob "mirror" = 0: every query runs as a kernel
    int max_clean = 256;           // largest batch answered on the host while the mirror is up to date (knob "mirror_max") ...
    int max_dirty = 32;            // ... and while it needs a refresh first (a large batch is then cheaper as one kernel)
    size_t max_bytes = (size_t)1 << 30; // most pinned host memory the planes may take (mlm_set_host_mirror_limit; knob "mirror_mb"): a map
                                   // that needs more is queried by kernels only (over_limit) — nothing is pinned behind the caller's back without bound
};
// the capacities of MlmDev that every frame slot gets (alloc_slot); the lists sized by need take theirs from MlmSlotCaps
struct MlmSlotPlan {
    unsigned int nb_cap = 0, node_cap = 0, chunk_cap = 0, mc_cap = 0, mvox_cap = 0, touch_cap = 0, mc_list_cap = 0;
};

// The members of mlm_handle that the plan decides (mlm_handle derives from this; the defaults are what a handle without knobs gets).
struct MlmHandlePlan {
    mlm_host::Q4 q_bs{};
    mlm_host::D3 t_bs{};
    std::vector<float> odds_table;
    size_t max_buckets = 0;
    unsigned int expand_block = 256;         // threads per k_expand_nodes block (128 and 64 measured slower)
    unsigned int sort_block = 256;           // threads per k_sort_contribs<1024> block
    unsigned int sort_grid = 256;            // blocks per frame of k_sort_contribs<1024> in a batch
    unsigned int rank_grid = 128;            // blocks per frame of k_rank in a batch (config 2 with two cells per wave: 87.5k frames/s, 64: 87.7k, 256: 86.4k,
                                             // 512: 84.7k; MLM_RANK_GRID)
    unsigned int chain_grid = 0;             // blocks per frame of k_chain_lanes (0: from the last confirmed frame's ranked cells; MLM_CHAIN_GRID)
    unsigned int collect_grid = 16;          // blocks per sub-list of k_collect_hits (grid-stride loop)
    unsigned int sc_block = 64;              // threads per block of the per-frame apply kernels: single-wave blocks are placed as soon as any wave
                                             // slot frees between Stage A's workgroups (config 2: 66.5k frames/s, 128: 64.1k, 256: 57.2k)
    bool sc_grid_fixed = false;              // MLM_SC_GRID given: do not adapt
    unsigned int sc_grid = 80;               // blocks per list of k_apply_voxelize (grid-stride loops; 40..120 measured equal, 160 3 % slower)
    int n_sets = MLM_SETS;     // slot sets in use (2 when three do not fit the device memory)
    int cu_split = 0;
    int cu_reserve = 0;
    bool use_sectors = true;   // Stage A by azimuth sector (mlm_kernels_sector.h); MLM_SECTORS=0: the cell-table path
    int sector_backoff_len = 16; // (MLM_SEC_BACKOFF)
    bool pool_grow = true;     // the block pool grows on demand (MLM_POOL_GROW=0: fixed at mlm_limits.max_blocks, MLM_ERR_CAPACITY when full)
    size_t frame_block_bound = 0; // most blocks one frame can create
    unsigned int tile_lds_bytes = 0; // dynamic LDS of k_tile
    int sec_threads = 512;           // threads of a column's workgroup (k_sector<.., 256 | 512>; MLM_SEC_THREADS)
    unsigned int single_rank_grid = 256;   // workgroups of a lone frame's k_rank<true> (ranking + chains; knob "single_rank_grid")
    unsigned int single_chain_grid = 64;  // workgroups of a lone frame's k_chain_lanes: 256 waves x 64 cells cover a dense VGA frame's ranked cells in one turn
    unsigned int single_apply_grid = 256; // workgroups of k_apply_single: a VGA frame's ~33 k voxel records, one per thread (more: in turns)
    unsigned int tile_grid = 0;      // workgroups of k_tile per frame of a batch: they walk the frame's touched tiles (MLM_TILE_GRID)
    unsigned int apply_lds_bytes = 0; // dynamic LDS of k_apply_tiles (mlm_apply_lds): 5 bytes per voxel of a tile, its layer and block tables
    unsigned int big_grid = 256;     // workgroups of k_sector_big per batch: one per CU (MLM_BIG_GRID)
    int ex_spec = 1;                 // frontier mode: a synchronous frame's map-dependent part is enqueued before its counts are known (explore_stage_bc_spec);
                                     // knob "ex_spec": 0 never, 2 with thresholds of zero (every frame misses: the test of the way back)
    int big_arm_len = 64;            // (MLM_BIG_ARM: 0 never schedules it)
    bool use_graph = true;       // (MLM_GRAPH=0: always the general submission)
    bool no_spread = false;      // the noise model never spreads a hit beyond its own cell (3 sigma < 1 cell everywhere, e.g. the reference's default
                                 // depth_noise_coe 1e-6): k_chain_lanes has nothing to do and is not launched
    int score_chunk = 0; // points per chunk of k_score (knob "score_chunk"; 0: automatic)
    unsigned int rays_grid = 1024; // most workgroups of k_rays (knob "rays_grid"): 2^20 rays are four per lane
    int render_tile = kRenderTileDefault; // (knob "render_tile")
    int clear_ahead = 1; // voxels a lane of k_clearance looks ahead (knob "clear_ahead": 1 or 4; DESIGN.md has the measurement)
    // Frame slots sized by NEED (sector-path handles, not frontier mode): the per-frame lists whose worst case is
    // "every awareness cell is a multi-kind hit" start at what a camera frame of max_points pixels needs and are doubled at a
    // drained point when a frame's Stage A runs out of room (grow_slots, like grow_pool for the block pool).  The cell-table path,
    // which a frame falls back to one at a time, gets ONE full-size set of those lists per handle, allocated at its first use.
    bool need_sized = false;
    MlmSlotCaps caps_worst, caps_now;
};

struct MlmPlan {
    int status = MLM_OK;   // a refusal: the status mlm_create returns ...
    std::string err;       // ... and its mlm_last_error
    mlm_limits lim{};      // the limits with their defaults filled in
    MlmDev P{};            // every scalar of the handle's parameter block (the pointers stay null: the device stages fill them)
    MlmHandlePlan H;
    MlmMirrorLimits mir;
    MlmSlotPlan slot;
    std::vector<float> sigma3;            // [nRho] 3 * sigma_in_dr(rho)
    std::vector<double> cos_phi, sin_phi; // [nPhi] of the column centres
    std::vector<uint32_t> sec_const;      // MlmDev::sec_const as k_sector lays it out
};

// the arguments mlm_create refuses before it makes a handle
inline bool mlm_plan_args_ok(const mlm_config &c) {
    return !(c.am_n_rho <= 1 || c.am_d_rho <= 0 || c.am_d_phi_deg <= 0 || c.am_d_z <= 0 || c.subbox_n <= 0 || c.subbox_d_xyz <= 0 || c.am_n_z_below < 0 ||
             c.am_n_z_over < 0);
}

// The widest noise spread: a point contributes to its centre cell and to (+d, -d) while d < 3 * sigma(rho) (map_awareness.cpp:149),
// 1 + 2 * dmax cells at most.
inline int mlm_spread_max(const std::vector<float> &sigma3) {
    const int nRho = (int)sigma3.size();
    int dmax = 0;
    for (int r = 0; r < nRho; ++r) {
        int d = 1;
        while ((float)d < sigma3[r] && r + d < nRho && d <= MLM_DIFF_RANGE) ++d;
        dmax = std::max(dmax, d - 1);
    }
    return dmax;
}

// dynamic LDS of a column's workgroup (k_sector, k_sector_big) with a cell table of `tab` entries
inline unsigned int mlm_col_lds(const MlmDev &P, unsigned int tab) {
    return mlm_sec_lds(tab, (unsigned int)(P.nZ * (P.explore ? P.nRho : P.RW)), (unsigned int)P.nRho, (unsigned int)P.nZ, P.explore != 0).total;
}
// Does a cell table of `tab` entries, worked on by `threads` threads, fit the sector path?  At most four entries per thread, the column's
// LDS within `lds_limit` (a CU's 160 KB less 1 KB of static LDS, as mlm_create and widen_sec_tab each spell it), and k_sector lists a
// column's miss cells in its cell table's space (implied for widen_sec_tab, whose smaller table held them already).  The callers add
// their own terms: mlm_create the rest of the envelope, widen_sec_tab its cap of 2048 entries and the large table's size.
inline bool mlm_sec_tab_fits(const MlmDev &P, unsigned int tab, int threads, unsigned int lds_limit) {
    return tab <= 4u * (unsigned int)threads && mlm_col_lds(P, tab) <= lds_limit && (size_t)P.nZ * P.RW * 64 <= (size_t)tab * sizeof(MlmSecCell);
}

// The worst-case and the initial capacities of a frame slot's lists.  Worst case: every awareness cell a multi-kind hit.  By need:
// what camera frames of max_points pixels produce, with room —
// config 2 (307 k pixels): 20 k hits, 8 k ranked cells, 260 k references, 730 k ordered kinds, 33 k voxel records per frame;
// config 3 (922 k pixels): 137 k hits, all ranked, 4.1 M references, 7.7 M kinds, 350 k records.
// max_contrib: most contributions one frame can make.
inline void mlm_slot_caps(const MlmDev &P, size_t max_points, size_t max_contrib, size_t max_buckets, bool need_sized, MlmSlotCaps &w, MlmSlotCaps &c) {
    const size_t NC = (size_t)P.nCells, Pn = max_points;
    w.hl = w.mt = w.vh = NC;
    // a frame touches at most one voxel per awareness cell, and no more voxels than its grid has
    w.rec = std::min<size_t>(NC, (size_t)P.lv_nx * P.lv_ny * P.lv_nz);
    // (a reference — one row of a group's lane mask — stands for at least one contribution; a cell's references start at a multiple
    // of MLM_SEC_REF_ALIGN, and a cell that needs references has at least two contributions)
    w.refs = std::min<size_t>(0xFFFFFFF0ull, max_contrib + (MLM_SEC_REF_ALIGN - 1) * std::min<size_t>(NC, max_contrib / 2) + 64);
    // segments are padded to 16 entries; a multi-kind cell has >= 2 contributions (refused beyond 2^32 by mlm_plan)
    w.sub = std::min<size_t>(0xFFFFFFF0ull, max_contrib + 15 * std::min<size_t>(NC, max_contrib / 2) + 64);
    // bucket-first table of a slot: room for the emulated container of a frame with up to 2 * max_points unique hit cells
    w.sbkt = std::min<size_t>(max_buckets, std::__detail::_Prime_rehash_policy()._M_next_bkt(4 * Pn + 2));
    c = w;
    if (!need_sized) return;
    c.hl = std::min(w.hl, std::max<size_t>(32768, Pn / 4));
    c.mt = c.hl;
    c.vh = c.hl;
    c.rec = std::min(w.rec, 2 * c.hl);
    c.refs = std::min(w.refs, std::max<size_t>(262144, 6 * Pn));
    c.sub = std::min(w.sub, std::max<size_t>(1u << 20, 10 * Pn));
    c.sbkt = std::min(w.sbkt, std::__detail::_Prime_rehash_policy()._M_next_bkt(2 * c.hl + 2));
}

// knob: bool(const char *name, long long &value) — true and the value if the knob is set (mlm_debug_set).  n_cu: the device's CUs.
template <class Knob> MlmPlan mlm_plan(const mlm_config &cfg, const mlm_limits *lim_in, Knob &&knob, int n_cu) {
    MlmPlan pl;
    MlmDev &P = pl.P;
    MlmHandlePlan &H = pl.H;
    mlm_limits &lim = pl.lim;
    long long kv = 0; // (value of a test / experiment knob, see mlm_debug_set)
    auto refuse = [&](int status, std::string text) {
        pl.status = status;
        pl.err = std::move(text);
    };
    if (!mlm_plan_args_ok(cfg)) return refuse(MLM_ERR_INVALID, ""), pl;
    if (lim_in) lim = *lim_in;
    if (lim.max_blocks <= 0) lim.max_blocks = 65536;
    if (lim.max_points <= 0) lim.max_points = 1280 * 720;
    if (lim.max_batch <= 0) lim.max_batch = 8;
    if (lim.max_batch > 64) lim.max_batch = 64;
    // (frontier mode: Stage A is batched too; the map-dependent part runs frame by frame, see run_slots)
    if ((long long)lim.max_points * 256 > 0xFFFFFFF0ll && cfg.use_exploration_frontiers)
        return refuse(MLM_ERR_UNSUPPORTED, "max_points too large for 32-bit miss insertion times"), pl;

    // ---- launch geometries and switches that are knobs only
    if (knob("expand_block", kv)) H.expand_block = (unsigned int)kv; // (whole waves in [64, 256]: knob_value_ok)
    if (knob("sort_block", kv)) H.sort_block = (unsigned int)kv;
    if (knob("sort_grid", kv)) H.sort_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("chain_grid", kv)) H.chain_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("rank_grid", kv)) H.rank_grid = (unsigned int)std::max(1, (int)kv);
    else if ((long long)cfg.am_n_rho * cfg.am_n_z_below > 4000) H.rank_grid = 384; // (fine maps order a hundred thousand cells per frame: config 3 128 blocks 33.0 us, 256: 31.0, 512: 29.2)
    if (knob("collect_grid", kv)) H.collect_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("sc_block", kv)) H.sc_block = (unsigned int)kv;
    if (knob("sc_grid", kv)) {
        H.sc_grid = (unsigned int)std::max(1, (int)kv);
        H.sc_grid_fixed = true;
    }
    if (knob("pool_grow", kv)) H.pool_grow = (int)kv != 0;
    if (knob("graph", kv)) H.use_graph = (int)kv != 0;
    if (knob("big_grid", kv)) H.big_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("big_arm", kv)) H.big_arm_len = std::max(0, (int)kv);
    if (knob("ex_spec", kv)) H.ex_spec = (int)kv;
    if (knob("single_chain_grid", kv)) H.single_chain_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("single_rank_grid", kv)) H.single_rank_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("single_apply_grid", kv)) H.single_apply_grid = (unsigned int)std::max(1, (int)kv);
    if (knob("mirror", kv)) pl.mir.enabled = (int)kv != 0;
    if (knob("mirror_mb", kv)) pl.mir.max_bytes = (size_t)std::max(0, (int)kv) << 20;
    if (knob("rays_grid", kv)) H.rays_grid = (unsigned int)kv;
    if (knob("render_tile", kv)) H.render_tile = (int)kv;
    if (knob("score_chunk", kv)) H.score_chunk = (int)kv;
    if (knob("clear_ahead", kv)) H.clear_ahead = (int)kv;
    if (knob("mirror_max", kv)) pl.mir.max_clean = std::max(0, (int)kv), pl.mir.max_dirty = std::min(pl.mir.max_dirty, pl.mir.max_clean);
    if (knob("slot_sets", kv)) H.n_sets = std::min(MLM_SETS, std::max(2, (int)kv));
    // Stage B+C (main stream) is the serial per-frame chain of short, latency-bound kernels; Stage A floods the
    // chip with wide kernels.  MLM_CU_SPLIT=k (default 0 = off) reserves the first k CUs for the main stream and
    // leaves the rest to Stage A, so that the chain is not stretched by queueing behind Stage A's waves.
    H.cu_split = knob("cu_split", kv) ? std::max(0, (int)kv) : 0;
    // MLM_CU_RESERVE=k: Stage A stays off the first k CUs, the main stream may use all of them
    if (knob("cu_reserve", kv)) H.cu_reserve = std::max(0, (int)kv);
    if (std::max(H.cu_split, H.cu_reserve) >= n_cu) // (Stage A's streams would get an empty CU mask: nothing of theirs could run)
        return refuse(MLM_ERR_INVALID, "knobs cu_split / cu_reserve must leave Stage A at least one of the device's " + std::to_string(n_cu) + " CUs"), pl;

    // ---- awareness constants, map_awareness.cpp:21-32
    P.dRho = cfg.am_d_rho;
    P.dPhi = cfg.am_d_phi_deg * M_PI / 180;
    P.dZ = cfg.am_d_z;
    P.nRho = cfg.am_n_rho;
    P.nPhi = static_cast<int>(360 / cfg.am_d_phi_deg);
    P.nZ = cfg.am_n_z_below + cfg.am_n_z_over + 1;
    P.zc = cfg.am_n_z_below;
    P.z_border_min = -(cfg.am_n_z_below * cfg.am_d_z) - 0.5 * cfg.am_d_z;
    P.nRhoPhi = P.nRho * P.nPhi;
    const long long ncells = (long long)P.nRhoPhi * P.nZ;
    if (ncells <= 0 || ncells > (1ll << 31) - 64) return refuse(MLM_ERR_UNSUPPORTED, "awareness map too large"), pl;
    if ((long long)lim.max_points * MLM_TIME_SLOTS > 0x7FFFFFF0ll) return refuse(MLM_ERR_UNSUPPORTED, "max_points too large for 32-bit insertion times"), pl;
    P.nCells = (int)ncells;
    P.RW = (P.nRho + 31) / 32;
    P.rw_m = mlm_host::strip_magic((unsigned int)P.RW); // (0 beyond 2^11 words: such a cylinder never takes the sector path, use_sectors below)
    P.nMissWords = P.nZ * P.nPhi * P.RW;
    P.visibility = cfg.use_raycasting != 0;
    // local constants, map_local.cpp:56-62,126-130 (float casts as mlmap.cpp:77-81)
    P.d_sub = cfg.subbox_d_xyz;
    P.d_sub_half = P.d_sub * 0.5;
    P.n = cfg.subbox_n;
    P.d_glb = P.d_sub * P.n;
    P.inv_dRho = 1.0 / P.dRho;
    P.inv_dPhi = 1.0 / P.dPhi;
    P.inv_dZ = 1.0 / P.dZ;
    P.inv_d_max = std::max(P.inv_dRho, std::max(P.inv_dPhi, P.inv_dZ));
    P.inv_d_sub = 1.0 / P.d_sub;
    P.inv_d_glb = 1.0 / P.d_glb;
    P.cells = P.n * P.n * P.n;
    P.lo_min = static_cast<float>(cfg.log_odds_min);
    P.lo_max = static_cast<float>(cfg.log_odds_max);
    P.lo_miss = static_cast<float>(cfg.measurement_miss);
    P.lo_sh = static_cast<float>(cfg.occupied_sh);
    // camera, mlmap.cpp:15-18 (float members) and mlmap.h:85-86
    P.cx = (float)cfg.cam_cx;
    P.cy = (float)cfg.cam_cy;
    P.fx = (float)cfg.cam_fx;
    P.fy = (float)cfg.cam_fy;
    P.inv_factor = 1.0 / 1000.0;
    P.inv_fx = 1.0 / (double)P.fx;
    P.inv_fy = 1.0 / (double)P.fy;
    P.record_awareness = lim.record_awareness;
    P.explore = cfg.use_exploration_frontiers != 0;
    P.max_blocks = lim.max_blocks;

    // T_bs, mlmap.cpp:22-25
    const double R[9] = {cfg.T_bs[0], cfg.T_bs[1], cfg.T_bs[2], cfg.T_bs[4], cfg.T_bs[5], cfg.T_bs[6], cfg.T_bs[8], cfg.T_bs[9], cfg.T_bs[10]};
    H.q_bs = mlm_host::q_from_R(R);
    H.t_bs = mlm_host::D3{cfg.T_bs[3], cfg.T_bs[7], cfg.T_bs[11]};

    // ---- tables (host libm, uploaded once)
    mlm_host::OddsModel om{cfg.am_d_rho, cfg.depth_noise_coe};
    H.odds_table.resize((size_t)21 * P.nRho);
    for (int d = -MLM_DIFF_RANGE; d <= MLM_DIFF_RANGE; ++d)
        for (int r = 0; r < P.nRho; ++r) H.odds_table[(size_t)(d + MLM_DIFF_RANGE) * P.nRho + r] = om.get_odds(d, (size_t)r);
    pl.sigma3.resize(P.nRho);
    for (int r = 0; r < P.nRho; ++r) pl.sigma3[r] = 3 * om.sigma_in_dr((size_t)r); // map_awareness.cpp:149
    {
        // The hit increment is the HOST libm's log10f(odd / (1 - odd)) in the reference (map_local.h:8, map_local.cpp:159).  If this
        // host's log10f is the one mlm_glibc_log10f restates (checked on the table's own logit arguments and a sweep of the range),
        // the kernels evaluate that restatement and every increment has the reference's float bits; else FP64 log10 rounded once.
        std::vector<float> ratios(H.odds_table.size());
        for (size_t i = 0; i < ratios.size(); ++i) ratios[i] = H.odds_table[i] / (1 - H.odds_table[i]);
        P.logit_exact = mlm_host::host_log10f_matches(ratios.data(), ratios.size()) ? 1 : 0;
        if (knob("logit_exact", kv)) P.logit_exact = P.logit_exact && (int)kv != 0;
    }
    pl.cos_phi.resize(P.nPhi);
    pl.sin_phi.resize(P.nPhi);
    for (int p = 0; p < P.nPhi; ++p) {
        const double center_phi = P.dPhi / 2 + (p * P.dPhi); // map_awareness.cpp:59
        pl.cos_phi[p] = std::cos(center_phi);
        pl.sin_phi[p] = std::sin(center_phi);
    }
    {
        const size_t nb = ((H.odds_table.size() + 3) & ~(size_t)3), nw = nb / 4 + ((pl.sigma3.size() + 3) & ~(size_t)3);
        pl.sec_const.assign(nw, 0u);
        for (size_t e = 0; e < H.odds_table.size(); ++e) ((uint8_t *)pl.sec_const.data())[e] = (uint8_t)mlm_sec_strength(H.odds_table[e]);
        std::memcpy(pl.sec_const.data() + nb / 4, pl.sigma3.data(), pl.sigma3.size() * sizeof(float));
        P.sec_const_words = (unsigned int)nw;
    }
    {
        // order-free hit values (MlmDev::hit_p / hit_inc): largest power of two up to the knob's (default 256) with which both tables
        // fit 16 MB; S1 takes 2 x 1.4 MB.
        unsigned int tn = 256;
        if (knob("hit_tab_n", kv)) tn = (unsigned int)kv;
        while (tn && 2 * H.odds_table.size() * tn * sizeof(float) > ((size_t)16 << 20)) tn >>= 1;
        P.hit_tab_n = tn;
    }

    // ---- k_bin_points: a point spreads into 1 + 2*dmax cells; the wider the spread, the more groups and distinct cells a block produces
    const int dmax = mlm_spread_max(pl.sigma3);
    H.no_spread = dmax == 0; // (a point only ever hits its own cell: no cell collects several kinds, nothing to rank or replay)
    P.node_lds = dmax > 4 ? 1024 : 448;
    P.agg_lds = dmax > 4 ? 512 : 256;
    // block size of k_bin_points and its LDS buffers (the sizes above are per 256 threads); experiment knobs
    P.bin_block = 256; // measured on config 2: 34.4k frames/s vs 33.6k with 512 and 31.9k with 1024
    if (knob("bin_block", kv)) P.bin_block = ((int)kv >= 1024) ? 1024u : ((int)kv >= 512 ? 512u : 256u);
    P.node_lds = P.node_lds * (P.bin_block / 256);
    P.agg_lds = P.agg_lds * (P.bin_block / 256);
    if (knob("node_lds", kv)) P.node_lds = (unsigned int)(int)kv;
    if (knob("agg_lds", kv)) P.agg_lds = (unsigned int)(int)kv; // power of two >= bin_block
    unsigned int lg = 0;
    while ((1u << lg) < P.agg_lds) ++lg;
    P.agg_shift = 32 - lg;
    P.bin_lds_bytes = P.node_lds * (unsigned int)sizeof(MlmNode) + P.agg_lds * (unsigned int)(sizeof(MlmCellAgg) + 4) + MLM_RAY_LDS * 16;
    if ((size_t)(2 * MLM_DIFF_RANGE + 1) * P.nRho * sizeof(float) > 64u * 1024u) // (k_chain keeps the odds table in LDS)
        return refuse(MLM_ERR_UNSUPPORTED, "am_n_Rho above 780 is not supported"), pl;

    // ---- sector path: LDS tables of one azimuth column (k_sector).  Cell table: a column rarely holds more hit cells than a
    // few per range step; references: (record, kind) pairs of its multi-kind cells.  A column that needs more makes
    // its frame fall back to the cell-table path.
    // (the hit cells of a column grow faster than its range steps — finer cells also mean more distinct cells per pixel footprint:
    // ~220 on config 2's 65 steps, ~1 000 on config 3's 130 — hence 6 entries per step for coarse maps, 12 for fine ones)
    unsigned int tab = 512;
    while (tab < (P.nRho > 100 ? 12u : 6u) * (unsigned int)P.nRho && tab < 2048u) tab <<= 1;
    if (knob("sec_tab", kv)) tab = (unsigned int)std::max(256, (int)kv); // power of two
    P.sec_tab = tab;
    // a column's workgroup: 256 threads where the table allows (at most 4 entries per thread, one thread per range step) — the
    // smaller workgroup and table leave wave slots and LDS of a CU to the other streams' kernels, which is worth more in the
    // pipeline (+5 % frames/s on config 2) than the 10 % the kernel loses alone
    H.sec_threads = (tab <= 1024u && P.nRho <= 256) ? 256 : 512;
    if (knob("sec_threads", kv)) H.sec_threads = ((int)kv <= 256 && tab <= 1024u && P.nRho <= 256) ? 256 : 512;
    if (P.sec_tab < (unsigned int)H.sec_threads) P.sec_tab = (unsigned int)H.sec_threads;
    if (knob("sec_backoff", kv)) H.sector_backoff_len = std::max(0, (int)kv);
    if (knob("sec_fail_every", kv)) P.sec_fail_every = (unsigned int)std::max(0, (int)kv);
    P.sec_lds_bytes = mlm_col_lds(P, P.sec_tab);
    {
        // second pass for the columns that overflow that table: the largest table (up to 4096 entries = 8 per thread) that
        // fits a CU's LDS — an S1 column has 2 665 cells in all, so no scene overflows it there
        unsigned int big = 4096;
        while (big > P.sec_tab && mlm_col_lds(P, big) > 159u * 1024u) big >>= 1;
        if (knob("sec_tab_big", kv)) big = (unsigned int)(int)kv; // (0 or <= MLM_SEC_TAB: no second pass)
        P.sec_tab_big = big > P.sec_tab && big <= 8u * MLM_SEC_THREADS ? big : 0u;
        P.sec_big_lds_bytes = P.sec_tab_big ? mlm_col_lds(P, P.sec_tab_big) : 0u;
    }
    {
        // frame-local voxel grid: the awareness cylinder (radius nRho*dRho, height nZ*dZ) plus four voxels each side, cut
        // into tiles over its whole height: the largest edge (8, 4, 2, 1 voxels) with at most 4096 voxels per tile — k_tile counts
        // them in LDS, and the workgroup that applies a tile walks its records a few per thread and frame (measured: config 3's
        // 0.05 m map, 110 layers, runs k_tile and k_apply_tiles 1.6x faster with 4x4 columns than with 8x8; config 2's 51 layers
        // are best at 8x8)
        const double Rc = P.nRho * P.dRho;
        P.lv_nx = P.lv_ny = 2 * (int)std::ceil(Rc / P.d_sub) + 10;
        P.lv_nz = (int)std::ceil(P.nZ * P.dZ / P.d_sub) + 10;
        P.tile_sh = 3;
        while (P.tile_sh > 0 && ((size_t)P.lv_nz << (2 * P.tile_sh)) > 4096) --P.tile_sh;
        // (a handle sized for frame-by-frame calls — the default max_batch of 8 or less — takes 4x4 columns: a lone frame's k_tile
        // lasts as long as its busiest tile, the sensor's own, and a quarter of that tile is done sooner: the 500-sample callback
        // 104 -> 95 us, a dense VGA frame 184 -> 172 us; long batches keep 8x8, worth 3 % of their throughput)
        if (lim.max_batch <= 8 && P.tile_sh > 2) P.tile_sh = 2;
        if (knob("tile_sh", kv)) P.tile_sh = std::min(3, std::max(0, (int)kv));
        const int edge = 1 << P.tile_sh;
        P.lv_nx += edge; // (the grid's origin is snapped down to a tile boundary: frame_setup)
        P.lv_ny += edge;
        P.n_tx = (P.lv_nx + edge - 1) / edge;
        P.n_tiles = P.n_tx * ((P.lv_ny + edge - 1) / edge);
        P.tile_words = (unsigned int)(P.nPhi + 31) / 32u; // a column's ray crosses a tile once: one descriptor slot per (tile, column)
        // (a camera frame reaches about a quarter of its grid's tiles: a workgroup takes eight candidate tiles, most of them empty.
        // Measured on config 2, profiles/r4g: 121 workgroups per frame 95.1 k frames/s, 80: 97.0 k, 60: 97.7 k, 45: 98.6 k, 32: 98.3 k —
        // the kernel alone is no faster with fewer, but its 29 KB of LDS per workgroup are the other streams' kernels' room)
        H.tile_grid = (unsigned int)std::max(32, std::min(P.n_tiles, P.n_tiles / 8 + 1));
        if (knob("tile_grid", kv)) H.tile_grid = (unsigned int)std::max(1, std::min(P.n_tiles, (int)kv));
        {   // blocks a tile overlaps: an extent of e voxels starting anywhere touches at most (e - 1) / n + 2 blocks of n
            const long long cx = (edge - 1) / P.n + 2, cz = (P.lv_nz - 1) / P.n + 2;
            P.tile_combos = (unsigned int)std::min<long long>((cx * cx * cz + 3) & ~3ll, 1ll << 20);
        }
        H.tile_lds_bytes = mlm_tile_lds((unsigned int)(edge * edge * P.lv_nz), (unsigned int)P.lv_nz, P.tile_combos).total;
        // (two grid heights of layers: frames of a range differ in z origin; launch_apply_tiles keeps a launch's spread within one)
        H.apply_lds_bytes = mlm_apply_lds((unsigned int)edge, 2u * (unsigned int)P.lv_nz, (unsigned int)P.n).total;
    }
    // (frontier mode: no tiles; its insertion times hold point index * 256 + ray step in 32 bits)
    // (k_sector lists a column's miss cells in its cell table's space; k_tile counts a voxel's misses and hits in 16 bits each:
    // no voxel may collect 2^16 cells — at most (d_sub / dRho + 2) (d_sub / dZ + 2) nPhi cell centres fall into one)
    const double cells_per_voxel = (std::ceil(P.d_sub / P.dRho) + 2) * (std::ceil(P.d_sub / P.dZ) + 2) * P.nPhi;
    H.use_sectors = P.bin_block == 256 && mlm_sec_tab_fits(P, P.sec_tab, H.sec_threads, 160u * 1024u - 1024u) && lim.max_points < (1 << MLM_SEC_CNT_BITS) && P.n <= 255 &&
                    P.nZ * P.nRho < 65536 &&
                    P.nZ < 32768 /* a column record holds z << 16 | rho below its top bit, MLM_SEC_OUTER (nZ * nRho < 65536 only implies it for nRho >= 2) */ &&
                    P.nRho <= 512 /* k_chain_lanes: 128 bytes of LDS per rho; k_sector: one thread per rho */ &&
                    P.nPhi <= 32 * MLM_TILE_WORDS /* k_tile: a tile's column mask */ &&
                    (P.explore ? P.nRho <= 256
                               : (((size_t)P.lv_nz << (2 * P.tile_sh)) <= 65536 && H.tile_lds_bytes <= 96u * 1024u && cells_per_voxel < 65536.0 &&
                                  P.n_tiles < (1 << 24) && P.lv_nz <= 1024 && H.apply_lds_bytes <= 150u * 1024u &&
                                  // (blocks one tile may overlap: their pool slots live in k_tile's LDS)
                                  P.tile_combos <= MLM_TILE_COMBOS));
    if (knob("sectors", kv)) H.use_sectors = H.use_sectors && (int)kv != 0;

    // ---- the emulated container can never hold more than nCells keys: bucket counts stay below the first libstdc++ prime >= 2*nCells
    const size_t NC = (size_t)P.nCells;
    H.max_buckets = std::__detail::_Prime_rehash_policy()._M_next_bkt(2 * NC + 2);
    {
        // most blocks ONE frame can create: those that overlap the frame-local voxel grid (every cell of the awareness cylinder
        // falls inside it, else the frame is redone / rejected)
        auto nb = [&](int nv) { return (long long)(nv + P.n - 1) / P.n + 1; };
        H.frame_block_bound = (size_t)std::min<long long>(nb(P.lv_nx) * nb(P.lv_ny) * nb(P.lv_nz), 1ll << 30);
    }

    // ---- frame slots sized by need (see MlmHandlePlan::need_sized; knob "need_slots" = 0: every list at its worst case, as up to round 4)
    H.need_sized = H.use_sectors && !P.explore;
    if (knob("need_slots", kv)) H.need_sized = H.need_sized && (int)kv != 0;
    const size_t max_contrib = (size_t)lim.max_points * (size_t)(1 + 2 * dmax); // most contributions one frame can make
    // (its padded form — segments of 16 entries, a multi-kind cell has >= 2 contributions — is MlmSlotCaps::sub's worst case)
    if (max_contrib > 0xFFFFFFF0ull || max_contrib + 15 * std::min<size_t>(NC, max_contrib / 2) + 64 > 0xFFFFFFF0ull)
        return refuse(MLM_ERR_UNSUPPORTED, "contribution buffer too large (frame slots: lower mlm_limits.max_batch or max_points)"), pl;
    mlm_slot_caps(P, (size_t)lim.max_points, max_contrib, H.max_buckets, H.need_sized, H.caps_worst, H.caps_now);
    // (256 work items per bin block; image edges and short lists add blocks: twice the quotient + 256)
    pl.slot.nb_cap = (unsigned int)((size_t)lim.max_points / 128 + 256);
    pl.slot.chunk_cap = pl.slot.nb_cap; // a column can at most get one run from every bin block
    pl.slot.node_cap = (unsigned int)(max_contrib / MLM_RAY_LISTS + 4096);
    pl.slot.touch_cap = (unsigned int)NC;
    pl.slot.mc_cap = (unsigned int)((size_t)P.nMissWords * 32 / MLM_RAY_LISTS + 4096);
    pl.slot.mvox_cap = (unsigned int)((size_t)P.nMissWords * 32 / MLM_RAY_LISTS + 512);
    pl.slot.mc_list_cap = H.use_sectors && !P.explore ? (unsigned int)NC : 0u; // unique miss cells of a frame (frontier mode: no tiles)
    return pl;
}
