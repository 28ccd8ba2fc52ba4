// mlm_mapview.h — the reference's query inlines (include/mlmap.h:142-295) over a HOST copy of the block planes: pure host code, no HIP.
// The library's host mirror (mlm_mirror.h) answers small query batches through it; tests/test_mapview.py builds it for the CPU with
// -fsanitize=address,undefined and holds every query kind to the oracle bit for bit.
//
// Layout mirrored: block slot s holds cells [s * cells, (s + 1) * cells) of log_odds / occupancy / inflate_occupancy, `collapsed[s]`
// marks a released block (vectors of size 1 in the reference: element 0 answers, mlmap.h:183-184,221-222); block keys are packed
// like the device's (three 21-bit biased indices) into an open-addressed table.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mlm_boxgrow.h"
#include "mlm_nearest.h"
#include "mlm_raywalk.h"
#include "mlm_score.h"
#include "mlm_sweep.h"

namespace mlm_host {

struct MapView {
    // geometry (map_local.cpp:56-62)
    double d_sub = 0, d_glb = 0, d_sub_half = 0;
    int n = 0, cells = 0;
    // the mirrored planes (not owned)
    const float *lo = nullptr;
    const uint8_t *occ = nullptr, *infl = nullptr, *col = nullptr;
    // block key -> slot
    std::vector<unsigned long long> tk;
    std::vector<int> ts;
    uint32_t tmask = 0;
    static constexpr unsigned long long kEmpty = 0xFFFFFFFFFFFFFFFFull;
    enum { FREE = 1, OCCUPIED = 0, UNKNOWN = -1 }; // mlmap.h:109-114

    static uint32_t mix(unsigned long long k) { // (the device's mlm_mix)
        k ^= k >> 33;
        k *= 0xff51afd7ed558ccdull;
        k ^= k >> 33;
        k *= 0xc4ceb9fe1a85ec53ull;
        k ^= k >> 33;
        return (uint32_t)k;
    }
    // a block index beyond the key's 21 bits per axis names no block of the map
    static bool key_ok(int gx, int gy, int gz) {
        return !((((unsigned int)gx + (1u << 20)) >> 21) || (((unsigned int)gy + (1u << 20)) >> 21) || (((unsigned int)gz + (1u << 20)) >> 21));
    }
    static unsigned long long pack(int gx, int gy, int gz) {
        return ((unsigned long long)(((uint32_t)gx + (1u << 20)) & 0x1FFFFFu) << 42) | ((unsigned long long)(((uint32_t)gy + (1u << 20)) & 0x1FFFFFu) << 21) |
               (unsigned long long)(((uint32_t)gz + (1u << 20)) & 0x1FFFFFu);
    }
    void table_reset(size_t cap_blocks) {
        size_t ht = 1024;
        while (ht < cap_blocks * 4) ht <<= 1;
        tk.assign(ht, kEmpty);
        ts.assign(ht, -1);
        tmask = (uint32_t)(ht - 1);
    }
    void table_clear() {
        tk.clear();
        ts.clear();
        tmask = 0;
    }
    void table_insert(int gx, int gy, int gz, int slot) {
        const unsigned long long key = pack(gx, gy, gz);
        uint32_t p = mix(key) & tmask;
        while (tk[p] != kEmpty) p = (p + 1) & tmask;
        tk[p] = key;
        ts[p] = slot;
    }
    int find(int gx, int gy, int gz) const {
        if (!key_ok(gx, gy, gz) || !tmask) return -1;
        const unsigned long long key = pack(gx, gy, gz);
        for (uint32_t p = mix(key) & tmask;; p = (p + 1) & tmask) {
            const unsigned long long k = tk[p];
            if (k == key) return ts[p];
            if (k == kEmpty) return -1;
        }
    }

    static int cvt_int(double v) { // x86 cvttsd2si (mlm_cvt_int)
        if (!(v > -2147483649.0 && v < 2147483648.0)) return (int)0x80000000;
        return (int)v;
    }
    static int mul(int a, int b) { return (int)((unsigned int)a * (unsigned int)b); } // (wraps like the hardware; INT_MIN * n is UB in C++)
    // get_global_idx / get_subbox_id, map_local.h:148-152,167-173 — two independent divisions per axis; a cell coordinate outside
    // [0, n) maps to id 0 (operator[] default-inserts in the reference)
    void voxel_of(double x, double y, double z, int g[3], int &cid) const {
        g[0] = cvt_int(std::floor(x / d_glb));
        g[1] = cvt_int(std::floor(y / d_glb));
        g[2] = cvt_int(std::floor(z / d_glb));
        const int cx = cvt_int(std::floor(x / d_sub) - mul(g[0], n));
        const int cy = cvt_int(std::floor(y / d_sub) - mul(g[1], n));
        const int cz = cvt_int(std::floor(z / d_sub) - mul(g[2], n));
        if (cx < 0 || cy < 0 || cz < 0 || cx >= n || cy >= n || cz >= n) cid = 0;
        else cid = cz * n * n + cy * n + cx;
    }
    // getOccupancy, mlmap.h:170-193
    int occupancy(double x, double y, double z) const {
        int g[3], cid;
        voxel_of(x, y, z, g, cid);
        const int slot = find(g[0], g[1], g[2]);
        if (slot < 0) return UNKNOWN;
        if (col[slot]) cid = 0; // occupancy.size() == 1 -> occupancy[0], mlmap.h:183-184
        const uint8_t r = occ[(size_t)slot * cells + cid];
        return r == 'o' ? OCCUPIED : (r == 'f' ? FREE : UNKNOWN);
    }
    // logit_inv, mlmap.h:40: pow(10, x) / (1 + pow(10, x)) in double, narrowed by getOdd's float return
    static float logit_inv(float L) {
        const double p = std::pow(10.0, (double)L);
        return (float)(p / (1 + p));
    }
    // getOdd(glb_id, subbox_id), mlmap.h:227-235
    float odd_at(int gx, int gy, int gz, int cid) const {
        const int slot = find(gx, gy, gz);
        if (slot < 0) return 0.5f;
        if (col[slot]) cid = 0; // log_odds.size() == 1 -> log_odds[0], mlmap.h:221-222
        return logit_inv(lo[(size_t)slot * cells + cid]);
    }
    // one step along direction dir of subbox_neighbors (map_local.cpp:77-120): order +z,-z,+y,-y,+x,-x
    void neighbor(int dir, int g[3], int &cid) const {
        int c[3];
        c[2] = cid / (n * n);
        c[1] = (cid - c[2] * n * n) / n;
        c[0] = cid - c[2] * n * n - c[1] * n;
        const int axis = 2 - dir / 2, step = (dir & 1) ? -1 : 1;
        c[axis] += step;
        if (c[axis] >= n) { // (block indices wrap like the hardware's: a NaN position sits at INT_MIN)
            g[axis] = (int)((unsigned int)g[axis] + 1u);
            c[axis] = 0;
        } else if (c[axis] < 0) {
            g[axis] = (int)((unsigned int)g[axis] - 1u);
            c[axis] = n - 1;
        }
        cid = c[2] * n * n + c[1] * n + c[0];
    }
    // mode 0: getOccupancy  1: getOccupancy(pos, inflate)  2: getInflateOccupancy  3: getOdd  4: getOddGrad (k_query's modes)
    void answer(int mode, const double *pos, int count, float inflate, int max_iter, void *out) const {
        for (int i = 0; i < count; ++i) {
            const double x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
            if (mode == 0) {
                ((int8_t *)out)[i] = (int8_t)occupancy(x, y, z);
            } else if (mode == 1) {
                // the 19-point stencil in the reference's order, mlmap.h:142-169; Vec3(+-inflate) promotes the float to double
                const double f = inflate;
                static const int8_t o[19][3] = {{0, 0, 0},  {0, 0, 1},   {0, 0, -1}, {0, 1, 0},   {0, -1, 0}, {1, 0, 0},  {-1, 0, 0},
                                                {-1, 1, 0}, {-1, -1, 0}, {1, 1, 0},  {1, -1, 0},  {0, -1, 1}, {0, -1, -1}, {0, 1, 1},
                                                {0, 1, -1}, {-1, 0, 1},  {-1, 0, -1}, {1, 0, 1},  {1, 0, -1}};
                int res = FREE;
                for (int k = 0; k < 19 && res == FREE; ++k)
                    if (occupancy(x + (o[k][0] ? (o[k][0] > 0 ? f : -f) : 0.0), y + (o[k][1] ? (o[k][1] > 0 ? f : -f) : 0.0),
                                  z + (o[k][2] ? (o[k][2] > 0 ? f : -f) : 0.0)) == OCCUPIED)
                        res = OCCUPIED;
                ((int8_t *)out)[i] = (int8_t)res;
            } else if (mode == 2) { // getInflateOccupancy, mlmap.h:195-211
                int g[3], cid;
                voxel_of(x, y, z, g, cid);
                const int slot = find(g[0], g[1], g[2]);
                int res = UNKNOWN;
                if (slot >= 0 && !col[slot] && infl[(size_t)slot * cells + cid] == 'o') res = OCCUPIED;
                ((int8_t *)out)[i] = (int8_t)res;
            } else if (mode == 3) {
                int g[3], cid;
                voxel_of(x, y, z, g, cid);
                ((float *)out)[i] = odd_at(g[0], g[1], g[2], cid);
            } else { // getOddGrad, mlmap.h:237-295
                int g[3], cid;
                voxel_of(x, y, z, g, cid);
                float min_odd = odd_at(g[0], g[1], g[2], cid);
                const float ori_odd = min_odd;
                int ng[6][3], ncid[6], mg[3] = {0, 0, 0}, mcid = 0;
                bool flag = false;
                for (int iter = 0; iter < max_iter && !flag; ++iter)
                    for (int d = 0; d < 6; ++d) {
                        if (iter == 0) {
                            ng[d][0] = g[0], ng[d][1] = g[1], ng[d][2] = g[2];
                            ncid[d] = cid;
                        }
                        neighbor(d, ng[d], ncid[d]); // (keeps searching along the original direction, mlmap.h:267-268)
                        const float tmp = odd_at(ng[d][0], ng[d][1], ng[d][2], ncid[d]);
                        if (tmp < min_odd) {
                            min_odd = tmp;
                            mg[0] = ng[d][0], mg[1] = ng[d][1], mg[2] = ng[d][2];
                            mcid = ncid[d];
                            flag = true;
                        }
                    }
                double r[3] = {0.0, 0.0, 0.0};
                if (flag) { // subbox_id2xyz_glb_vec, map_local.h:208-213
                    const int cz = mcid / (n * n), cy = (mcid - cz * n * n) / n, cx = mcid - cz * n * n - cy * n;
                    const double s = (double)(ori_odd - min_odd);
                    r[0] = ((mg[0] * d_glb + cx * d_sub + d_sub_half) - x) * s;
                    r[1] = ((mg[1] * d_glb + cy * d_sub + d_sub_half) - y) * s;
                    r[2] = ((mg[2] * d_glb + cz * d_sub + d_sub_half) - z) * s;
                }
                ((double *)out)[3 * (size_t)i] = r[0];
                ((double *)out)[3 * (size_t)i + 1] = r[1];
                ((double *)out)[3 * (size_t)i + 2] = r[2];
            }
        }
    }
    // mlm_query_rays on the mirrored planes: the walk of mlm_raywalk.h over the classes getOccupancy / getInflateOccupancy return at
    // the voxels (a released block answers from element 0, its inflated class is UNKNOWN; an absent block is UNKNOWN).  One table
    // probe per block crossed.
    struct RayClasses {
        const MapView &v;
        int slot = -1, fixed = 4; // fixed: the class of every voxel of an absent or released block
        bool whole = true;
        static int occ_bits(uint8_t r) { return r == 'o' ? 1 : (r == 'f' ? 0 : 4); }
        int operator()(const int g[3], const int c[3], bool new_block) {
            if (new_block) {
                slot = v.find(g[0], g[1], g[2]);
                whole = slot < 0 || v.col[slot];
                fixed = slot < 0 ? 4 : occ_bits(v.occ[(size_t)slot * v.cells]);
            }
            if (whole) return fixed;
            const size_t at = (size_t)slot * v.cells + (size_t)((c[2] * v.n + c[1]) * v.n + c[0]);
            return occ_bits(v.occ[at]) | (v.infl[at] == 'o' ? 2 : 0);
        }
    };
    void ray(const double p0[3], const double p1[3], int flags, MlmRayResult &o) const {
        RayClasses cls{*this};
        mlm_ray_walk(p0, p1, d_sub, n, flags, cls, o);
    }
    // a batch, any output may be null (mlm_query_rays' layout)
    void rays(const double *p0, const double *p1, int count, int flags, int8_t *status, int32_t *voxel3, double *t, int32_t *n_steps,
              int32_t *n_unknown) const {
        for (int i = 0; i < count; ++i) {
            MlmRayResult o;
            ray(p0 + 3 * (size_t)i, p1 + 3 * (size_t)i, flags, o);
            if (status) status[i] = (int8_t)o.status;
            if (voxel3)
                for (int a = 0; a < 3; ++a) voxel3[3 * (size_t)i + a] = o.voxel[a];
            if (t) t[i] = o.t;
            if (n_steps) n_steps[i] = o.n_steps;
            if (n_unknown) n_unknown[i] = o.n_unknown;
        }
    }
    // mlm_query_boxes on the mirrored planes: the growth of mlm_boxgrow.h over the same classes.  The scan walks the box block by
    // block: one table probe per block touched, no plane memory for an absent or released block.
    struct BoxScan {
        const MapView &v;
        static long long fdiv(long long a, long long n) { return a >= 0 ? a / n : -((-a + n - 1) / n); }
        void operator()(const int32_t lo[3], const int32_t hi[3], int flags, bool full, long long &n_unknown, long long &n_obstacle) const {
            const long long n = v.n;
            long long g0[3], g1[3];
            for (int a = 0; a < 3; ++a) {
                g0[a] = fdiv(lo[a], n);
                g1[a] = fdiv(hi[a], n);
            }
            for (long long gz = g0[2]; gz <= g1[2]; ++gz)
                for (long long gy = g0[1]; gy <= g1[1]; ++gy)
                    for (long long gx = g0[0]; gx <= g1[0]; ++gx) {
                        const long long g[3] = {gx, gy, gz};
                        long long c0[3], c1[3], cnt = 1; // the cells of this block inside the box
                        for (int a = 0; a < 3; ++a) {
                            c0[a] = std::max<long long>(lo[a], g[a] * n) - g[a] * n;
                            c1[a] = std::min<long long>(hi[a], g[a] * n + n - 1) - g[a] * n;
                            cnt *= c1[a] - c0[a] + 1;
                        }
                        const int slot = v.find((int)gx, (int)gy, (int)gz);
                        if (slot < 0 || v.col[slot]) {
                            const int bits = slot < 0 ? 4 : RayClasses::occ_bits(v.occ[(size_t)slot * v.cells]);
                            if (bits & 4) n_unknown += cnt;
                            if (bits & flags) n_obstacle += cnt;
                        } else {
                            for (long long cz = c0[2]; cz <= c1[2]; ++cz)
                                for (long long cy = c0[1]; cy <= c1[1]; ++cy)
                                    for (long long cx = c0[0]; cx <= c1[0]; ++cx) {
                                        const size_t at = (size_t)slot * v.cells + (size_t)((cz * n + cy) * n + cx);
                                        const int bits = RayClasses::occ_bits(v.occ[at]) | (v.infl[at] == 'o' ? 2 : 0);
                                        n_unknown += (bits >> 2) & 1;
                                        n_obstacle += (bits & flags) ? 1 : 0;
                                    }
                        }
                        if (!full && n_obstacle) return;
                    }
        }
    };
    void box(const int32_t b6[6], int flags, const MlmBoxLimits &L, MlmBoxResult &o) const {
        BoxScan scan{*this};
        mlm_box_grow(b6, flags, L, scan, o);
    }
    // a batch, any output may be null (mlm_query_boxes' layout)
    void boxes(const int32_t *box6, int count, int flags, const MlmBoxLimits &L, int8_t *status, int32_t *out6, uint8_t *closed, int64_t *table) const {
        for (int i = 0; i < count; ++i) {
            MlmBoxResult o;
            box(box6 + 6 * (size_t)i, flags, L, o);
            if (status) status[i] = (int8_t)o.status;
            if (out6)
                for (int k = 0; k < 6; ++k) out6[6 * (size_t)i + k] = o.box[k];
            if (closed) closed[i] = (uint8_t)o.closed;
            if (table)
                for (int k = 0; k < 4; ++k) table[4 * (size_t)i + k] = o.row[k];
        }
    }
    // mlm_query_nearest on the mirrored planes: the search of mlm_nearest.h over the same classes.  One table probe per block that the
    // bounds let through, no plane memory for an absent or released block.
    struct NearScan {
        const MapView &v;
        int slot = -1;
        int probe(const int g[3]) {
            slot = v.find(g[0], g[1], g[2]);
            if (slot < 0) return 4;
            if (v.col[slot]) return RayClasses::occ_bits(v.occ[(size_t)slot * v.cells]);
            return -1;
        }
        unsigned long long scan(const MlmNearPoint &p, const int g[3], const int c0[3], const int c1[3], int flags) const {
            unsigned long long best = MLM_NEAR_NOKEY;
            for (int cz = c0[2]; cz <= c1[2]; ++cz)
                for (int cy = c0[1]; cy <= c1[1]; ++cy)
                    for (int cx = c0[0]; cx <= c1[0]; ++cx) {
                        const size_t at = (size_t)slot * v.cells + (size_t)((cz * v.n + cy) * v.n + cx);
                        int bits = RayClasses::occ_bits(v.occ[at]);
                        if (flags & 2) bits |= v.infl[at] == 'o' ? 2 : 0; // (infl is read only when INFL is selected, as in k_nearest)
                        if (!(bits & flags)) continue;
                        const int32_t o[3] = {g[0] * v.n + cx, g[1] * v.n + cy, g[2] * v.n + cz};
                        best = std::min(best, mlm_near_voxel_key(p, o));
                    }
            return best;
        }
    };
    void nearest_one(const double pos[3], int max_dist, int flags, MlmNearResult &o) const {
        NearScan vox{*this};
        mlm_near_search(pos, d_sub, n, max_dist, flags, vox, o);
    }
    // a batch, any output may be null (mlm_query_nearest's layout)
    void nearest(const double *pos, int count, int max_dist, int flags, int8_t *status, int32_t *voxel3, int32_t *delta3, int64_t *sq,
                 double *dist) const {
        for (int i = 0; i < count; ++i) {
            MlmNearResult o;
            nearest_one(pos + 3 * (size_t)i, max_dist, flags, o);
            if (status) status[i] = (int8_t)o.status;
            for (int a = 0; a < 3; ++a) {
                if (voxel3) voxel3[3 * (size_t)i + a] = o.voxel[a];
                if (delta3) delta3[3 * (size_t)i + a] = o.delta[a];
            }
            if (sq) sq[i] = o.sq;
            if (dist) dist[i] = o.dist;
        }
    }
    // mlm_query_sweeps on the mirrored planes: the walk of mlm_sweep.h over the same classes.  The cap's voxels are looked up one by
    // one (the block of the previous one is kept); the start voxel's ball is NearScan's.
    struct SweepVox {
        const MapView &v;
        const uint32_t *tab; // the column table of the call's radius
        int cols;
        RayClasses cls;
        NearScan near;
        int bg[3] = {0, 0, 0}, slot = -1; // the block of the last cap voxel
        bool have = false;
        SweepVox(const MapView &view, const uint32_t *t, int L) : v(view), tab(t), cols(L), cls{view}, near{view} {}
        int centre(const int g[3], const int c[3], bool new_block) { return cls(g, c, new_block); }
        unsigned long long start(const MlmRayState &S, int r, int flags) {
            const int u[3] = {S.g[0] * v.n + S.c[0], S.g[1] * v.n + S.c[1], S.g[2] * v.n + S.c[2]};
            return mlm_sweep_start(u, v.n, r, flags, near);
        }
        unsigned long long cap(const MlmRayState &S, int axis, int s, bool, int, int flags) {
            unsigned long long best = MLM_SWEEP_NOKEY;
            for (int j = 0; j < cols; ++j) {
                int off[3], g[3], c[3];
                const unsigned long long key = mlm_sweep_column_key(tab[j], axis, s, off);
                for (int a = 0; a < 3; ++a) {
                    g[a] = S.g[a];
                    c[a] = S.c[a] + off[a];
                    while (c[a] < 0) c[a] += v.n, --g[a];
                    while (c[a] >= v.n) c[a] -= v.n, ++g[a];
                }
                if (!have || g[0] != bg[0] || g[1] != bg[1] || g[2] != bg[2]) {
                    slot = v.find(g[0], g[1], g[2]);
                    bg[0] = g[0], bg[1] = g[1], bg[2] = g[2];
                    have = true;
                }
                int bits;
                if (slot < 0) bits = 4;
                else if (v.col[slot]) bits = RayClasses::occ_bits(v.occ[(size_t)slot * v.cells]);
                else {
                    const size_t at = (size_t)slot * v.cells + (size_t)((c[2] * v.n + c[1]) * v.n + c[0]);
                    bits = RayClasses::occ_bits(v.occ[at]);
                    if (flags & 2) bits |= v.infl[at] == 'o' ? 2 : 0; // (infl is read only when INFL is selected, as in k_sweeps)
                }
                if ((bits & flags) && key < best) best = key;
            }
            return best;
        }
    };
    // tab: mlm_sweep_table(radius), L columns
    void sweep_one(const double p0[3], const double p1[3], int radius, int flags, const uint32_t *tab, int L, MlmSweepResult &o) const {
        SweepVox vox(*this, tab, L);
        mlm_sweep_walk(p0, p1, d_sub, n, radius, flags, vox, o);
    }
    // a batch, any output may be null (mlm_query_sweeps' layout)
    void sweep(const double *p0, const double *p1, int count, int radius, int flags, int8_t *status, int32_t *voxel3, double *t, int32_t *n_steps,
               int32_t *n_unknown, int32_t *hit3, int32_t *hit_sq) const {
        std::vector<uint32_t> tab(MLM_SWEEP_MAX_COLS);
        const int L = mlm_sweep_table(radius, tab.data());
        for (int i = 0; i < count; ++i) {
            MlmSweepResult o;
            sweep_one(p0 + 3 * (size_t)i, p1 + 3 * (size_t)i, radius, flags, tab.data(), L, o);
            if (status) status[i] = (int8_t)o.ray.status;
            for (int a = 0; a < 3; ++a) {
                if (voxel3) voxel3[3 * (size_t)i + a] = o.ray.voxel[a];
                if (hit3) hit3[3 * (size_t)i + a] = o.hit[a];
            }
            if (t) t[i] = o.ray.t;
            if (n_steps) n_steps[i] = o.ray.n_steps;
            if (n_unknown) n_unknown[i] = o.ray.n_unknown;
            if (hit_sq) hit_sq[i] = o.hit_sq;
        }
    }
    // mlm_score_poses on the mirrored planes: the rule of mlm_score.h, pose by pose and point by point, over the same classes (one
    // table probe per run of points inside one block).  Without classes nothing of the planes is read: a view that has only d_sub and
    // n answers a field-only call.  F.sqdist null: no field.  All eight words of every row are written.
    template <bool CLASSES, bool FIELD> void score_rows(const double *pts_s, int n_pts, const double *T_ws, int n_poses, const MlmScoreField &F, int64_t *table) const {
        for (int k = 0; k < n_poses; ++k) {
            unsigned long long acc[MLM_SCORE_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
            RayClasses cls{*this};
            MlmScoreBlock B{};
            for (int j = 0; j < n_pts; ++j)
                mlm_score_pair<CLASSES, FIELD>(T_ws + 12 * (size_t)k, pts_s + 3 * (size_t)j, d_sub, n, F, cls, B, acc);
            for (int w = 0; w < MLM_SCORE_WORDS; ++w) table[MLM_SCORE_WORDS * (size_t)k + w] = (int64_t)acc[w];
        }
    }
    void score(const double *pts_s, int n_pts, const double *T_ws, int n_poses, bool classes, const MlmScoreField &F, int64_t *table) const {
        if (classes && F.sqdist) score_rows<true, true>(pts_s, n_pts, T_ws, n_poses, F, table);
        else if (classes) score_rows<true, false>(pts_s, n_pts, T_ws, n_poses, F, table);
        else score_rows<false, true>(pts_s, n_pts, T_ws, n_poses, F, table);
    }
};

// Where the device map may differ from the mirror: up to kMax boxes of block indices (inclusive bounds) or "anywhere".  The rule the
// refresh relies on: a block inside ANY box ever marked since the last clear() is covered() — boxes are only merged into larger ones.
struct DirtyBoxes {
    static constexpr int kMax = 16;
    bool all = true;
    int n = 0;
    int lo[kMax][3], hi[kMax][3];
    void mark_all() {
        all = true;
        n = 0;
    }
    void clear() {
        all = false;
        n = 0;
    }
    void mark(const int blo[3], const int bhi[3]) {
        if (all) return;
        for (int k = 0; k < n; ++k) { // already covered?
            bool in = true;
            for (int a = 0; a < 3; ++a) in = in && blo[a] >= lo[k][a] && bhi[a] <= hi[k][a];
            if (in) return;
        }
        if (n == kMax) { // the list is full: one box around everything recorded so far
            for (int k = 1; k < n; ++k)
                for (int a = 0; a < 3; ++a) {
                    lo[0][a] = lo[k][a] < lo[0][a] ? lo[k][a] : lo[0][a];
                    hi[0][a] = hi[k][a] > hi[0][a] ? hi[k][a] : hi[0][a];
                }
            n = 1;
        }
        for (int a = 0; a < 3; ++a) {
            lo[n][a] = blo[a];
            hi[n][a] = bhi[a];
        }
        n++;
    }
    // a box of world coordinates with one block of margin each side; anything not finite or beyond the key range: "anywhere"
    void mark_world(const double wlo[3], const double whi[3], double d_glb) {
        int blo[3], bhi[3];
        for (int a = 0; a < 3; ++a) {
            const double l = std::floor(wlo[a] / d_glb) - 1.0, u = std::floor(whi[a] / d_glb) + 1.0;
            if (!(l > -1048000.0 && u < 1048000.0 && l <= u)) { // (NaN fails)
                mark_all();
                return;
            }
            blo[a] = (int)l;
            bhi[a] = (int)u;
        }
        mark(blo, bhi);
    }
    bool covered(int gx, int gy, int gz) const { // (what k_mirror_refresh evaluates per block)
        if (all) return true;
        for (int k = 0; k < n; ++k)
            if (gx >= lo[k][0] && gx <= hi[k][0] && gy >= lo[k][1] && gy <= hi[k][1] && gz >= lo[k][2] && gz <= hi[k][2]) return true;
        return false;
    }
};

} // namespace mlm_host
