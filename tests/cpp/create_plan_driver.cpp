// Test driver for mlm_plan (mlmapping_amd/csrc/mlm_plan.h): everything mlm_create decides without the device, built by
// tests/test_create_plan.py with g++ -fsanitize=address,undefined.  Reads cases from stdin, one statement per line:
//   case NAME | cfg FIELD VALUE | cfg T_bs INDEX VALUE | lim FIELD VALUE | knob NAME VALUE | ncu N | run
// and prints, per `run`, "case NAME", the plan as "name value" rows (doubles with 17 digits) and "end".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "mlm_plan.h"

static void I(const char *name, long long v) { std::printf("%s %lld\n", name, v); }
static void D(const char *name, double v) { std::printf("%s %.17g\n", name, v); }
#define PI(m) I("P." #m, (long long)P.m)
#define PD(m) D("P." #m, (double)P.m)
#define HI(m) I("h." #m, (long long)H.m)

static void print_caps(const char *pre, const MlmSlotCaps &c) {
    const std::pair<const char *, size_t> m[] = {{"hl", c.hl}, {"mt", c.mt}, {"vh", c.vh}, {"rec", c.rec}, {"refs", c.refs}, {"sub", c.sub}, {"sbkt", c.sbkt}};
    for (const auto &e : m) std::printf("%s.%s %zu\n", pre, e.first, e.second);
}

static void print_plan(const MlmPlan &pl) {
    const MlmDev &P = pl.P;
    const MlmHandlePlan &H = pl.H;
    I("status", pl.status);
    std::printf("err %s\n", pl.err.c_str());
    I("lim.max_blocks", pl.lim.max_blocks), I("lim.max_points", pl.lim.max_points), I("lim.max_batch", pl.lim.max_batch), I("lim.record_awareness", pl.lim.record_awareness);
    if (pl.status != MLM_OK) return;
    PD(dRho), PD(dPhi), PD(dZ), PD(z_border_min);
    PI(nRho), PI(nPhi), PI(nZ), PI(zc), PI(nRhoPhi), PI(nCells), PI(RW), PI(rw_m), PI(nMissWords), PI(visibility), PI(logit_exact);
    PD(d_sub), PD(d_glb), PD(d_sub_half), PD(inv_dRho), PD(inv_dPhi), PD(inv_dZ), PD(inv_d_sub), PD(inv_d_glb);
    PI(n), PI(cells), PD(lo_min), PD(lo_max), PD(lo_miss), PD(lo_sh);
    PD(cx), PD(cy), PD(fx), PD(fy), PD(inv_factor), PD(inv_fx), PD(inv_fy), PD(inv_d_max);
    PI(sec_const_words), PI(hit_tab_n), PI(record_awareness), PI(max_blocks), PI(explore);
    PI(node_lds), PI(agg_lds), PI(agg_shift), PI(bin_lds_bytes), PI(bin_block);
    PI(sec_tab), PI(sec_lds_bytes), PI(sec_tab_big), PI(sec_big_lds_bytes), PI(sec_fail_every);
    PI(lv_nx), PI(lv_ny), PI(lv_nz), PI(tile_sh), PI(n_tx), PI(n_tiles), PI(tile_combos), PI(tile_words);
    // (the template block of the handle carries no slot capacities: alloc_slot sets them in the slots' copies)
    PI(nb_cap), PI(node_cap), PI(chunk_cap), PI(mc_cap), PI(mvox_cap), PI(touch_cap), PI(mc_list_cap);
    I("S.nb_cap", pl.slot.nb_cap), I("S.node_cap", pl.slot.node_cap), I("S.chunk_cap", pl.slot.chunk_cap), I("S.mc_cap", pl.slot.mc_cap);
    I("S.mvox_cap", pl.slot.mvox_cap), I("S.touch_cap", pl.slot.touch_cap), I("S.mc_list_cap", pl.slot.mc_list_cap);
    HI(use_sectors), HI(no_spread), HI(need_sized), HI(sec_threads), HI(tile_grid), HI(tile_lds_bytes), HI(apply_lds_bytes), HI(rank_grid);
    HI(expand_block), HI(sort_block), HI(sort_grid), HI(chain_grid), HI(collect_grid), HI(sc_block), HI(sc_grid), HI(sc_grid_fixed), HI(cu_split), HI(cu_reserve);
    HI(sector_backoff_len), HI(pool_grow), HI(use_graph), HI(big_grid), HI(big_arm_len), HI(ex_spec), HI(single_chain_grid), HI(single_rank_grid), HI(single_apply_grid);
    HI(rays_grid), HI(render_tile), HI(score_chunk), HI(frame_block_bound), HI(max_buckets), HI(n_sets);
    I("h.mir.enabled", pl.mir.enabled), I("h.mir.max_bytes", (long long)pl.mir.max_bytes), I("h.mir.max_clean", pl.mir.max_clean), I("h.mir.max_dirty", pl.mir.max_dirty);
    D("h.q_bs.w", H.q_bs.w), D("h.q_bs.x", H.q_bs.x), D("h.q_bs.y", H.q_bs.y), D("h.q_bs.z", H.q_bs.z), D("h.t_bs.x", H.t_bs.x), D("h.t_bs.y", H.t_bs.y), D("h.t_bs.z", H.t_bs.z);
    print_caps("caps_worst", H.caps_worst);
    print_caps("caps_now", H.caps_now);
    std::printf("line1 [create] sector path %d: LDS %u bytes per column (table %u entries), frame-local grid %d x %d x %d in %d tiles of edge %d (%u bytes of LDS each)\n",
                (int)H.use_sectors, P.sec_lds_bytes, P.sec_tab, P.lv_nx, P.lv_ny, P.lv_nz, P.n_tiles, 1 << P.tile_sh, H.tile_lds_bytes);
    // ---- what the invariants of the test need beyond the scalars
    I("spread_max", mlm_spread_max(pl.sigma3));
    std::printf("sigma3");
    for (float s : pl.sigma3) std::printf(" %.9g", (double)s);
    std::printf("\n");
    I("tables.odds", (long long)H.odds_table.size()), I("tables.cos_phi", (long long)pl.cos_phi.size()), I("tables.sin_phi", (long long)pl.sin_phi.size());
    I("tables.sec_const", (long long)pl.sec_const.size());
    {
        const MlmSecLds L = mlm_sec_lds(P.sec_tab, (uint32_t)(P.nZ * (P.explore ? P.nRho : P.RW)), (uint32_t)P.nRho, (uint32_t)P.nZ, P.explore != 0);
        std::printf("sec_lds %u %u %u %u %u %u %u %u %u %u %u %u\n", L.tab, L.chunk, L.odds, L.sigma, L.miss, L.rays, L.multi, L.ray_p0, L.vox, L.aux, L.total, L.occ);
        I("col_lds", mlm_col_lds(P, P.sec_tab));
        const MlmTileLds T = mlm_tile_lds((uint32_t)(P.lv_nz << (2 * P.tile_sh)), (uint32_t)P.lv_nz, P.tile_combos);
        std::printf("tile_lds %u %u %u %u %u %u\n", T.cnt, T.place, T.desc, T.slot, T.ztab, T.total);
    }
    // widen_sec_tab's question for the tables it could reach: twice and four times the entries, with its rule for the thread count
    int nt = H.sec_threads;
    for (unsigned int m = 2; m <= 4; m *= 2) {
        const unsigned int tab = P.sec_tab * m;
        nt = nt == 256 && tab <= 1024u ? 256 : 512;
        std::printf("widen %u %d %d\n", tab, nt, (int)mlm_sec_tab_fits(P, tab, nt, 159u * 1024u));
    }
}

int main() {
    mlm_config cfg{};
    mlm_limits lim{};
    std::map<std::string, long long> knobs;
    int ncu = 256;
    std::string line, name;
    auto knob = [&](const char *k, long long &v) {
        const auto it = knobs.find(k);
        if (it == knobs.end()) return false;
        v = it->second;
        return true;
    };
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, f;
        in >> op;
        if (op == "case") {
            in >> name;
            cfg = mlm_config{};
            lim = mlm_limits{};
            knobs.clear();
        } else if (op == "cfg") {
            in >> f;
#define CD(m) if (f == #m) in >> cfg.m
            CD(am_d_rho); CD(am_d_phi_deg); CD(am_d_z); CD(am_n_rho); CD(am_n_z_below); CD(am_n_z_over); CD(use_raycasting); CD(depth_noise_coe);
            CD(subbox_d_xyz); CD(subbox_n); CD(use_exploration_frontiers); CD(log_odds_min); CD(log_odds_max); CD(measurement_hit); CD(measurement_miss);
            CD(occupied_sh); CD(inflate_n); CD(inflate_global_n); CD(apply_inflate); CD(sample_cnt); CD(cam_cx); CD(cam_cy); CD(cam_fx); CD(cam_fy);
#undef CD
            if (f == "T_bs") {
                int i = 0;
                in >> i;
                if (i < 0 || i >= 16) return 2;
                in >> cfg.T_bs[i];
            }
        } else if (op == "lim") {
            in >> f;
            if (f == "max_blocks") in >> lim.max_blocks;
            if (f == "max_points") in >> lim.max_points;
            if (f == "max_batch") in >> lim.max_batch;
            if (f == "record_awareness") in >> lim.record_awareness;
        } else if (op == "knob") {
            long long v = 0;
            in >> f >> v;
            knobs[f] = v;
        } else if (op == "ncu") {
            in >> ncu;
        } else if (op == "run") {
            std::printf("case %s\n", name.c_str());
            print_plan(mlm_plan(cfg, &lim, knob, ncu));
            std::printf("end\n");
        } else if (!op.empty()) {
            return 2;
        }
        if (in.fail()) return 3;
    }
    return 0;
}
