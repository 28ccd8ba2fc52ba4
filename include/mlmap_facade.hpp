// mlmap_facade.hpp — header-only C++ class with the reference's public `mlmap` names (include/mlmap.h:105-139)
// on top of the C ABI of mlmap_hip.h, so that a ROS host (or a planner that today does `#include <mlmap.h>`)
// can swap the CPU maps for the MI355X path without touching its call sites.
//
// No Eigen / ROS dependency: Vec3 is any type with operator[](int) -> double (Eigen::Vector3d qualifies).
// Not part of the hot path: every method is a thin forward to one mlm_* call.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "mlmap_hip.h"

namespace mlmap_hip {

struct Vec3d {
    double v[3];
    double operator[](int i) const { return v[i]; }
    double &operator[](int i) { return v[i]; }
};

// What visualisers read by iterating local_map->observed_group_map (src/rviz_vis.cpp:267-327, src/mlmap.cpp:226-276): a host
// SNAPSHOT with the reference's member names (include/map_local.h:42-60,92,201-213), so that code written against
// `local_map_cartesian *localmap` — `for (auto it = localmap->observed_group_map.begin(); ...)`, `it->second.inflate_occupancy`,
// `it->second.frontier`, `localmap->subbox_id2xyz_glb(it->first, id)` — compiles against `mlmap::local_map_snapshot().get()`.
struct Vec3I {
    int v[3];
    int operator[](int i) const { return v[i]; }
    int &operator[](int i) { return v[i]; }
    int size() const { return 3; }
    bool operator==(const Vec3I &o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
};
struct PointF { // pcl::PointXYZ's payload
    float x, y, z;
};
struct local_map_view {
    struct VectorHasher { // include/map_local.h:42-52
        int operator()(const Vec3I &V) const {
            int hash = V.size();
            hash ^= V[0] + 0x9e3779b9 + (hash << 6) + (hash >> 2);
            hash ^= V[1] + 0x9e3779b9 + (hash << 6) + (hash >> 2);
            hash ^= V[2] + 0x9e3779b9 + (hash << 6) + (hash >> 2);
            return hash;
        }
    };
    struct subbox { // include/map_local.h:53-60; a released block holds ONE element per vector (map_local.cpp:221-226)
        std::vector<char> occupancy, inflate_occupancy;
        std::vector<float> log_odds;
        std::unordered_set<int> frontier;
    };
    std::unordered_map<Vec3I, subbox, VectorHasher> observed_group_map;
    double map_dxyz_obv_sub = 0, map_dxyz_obv_glb = 0, map_dxyz_obv_sub_half = 0;
    int subbox_nxyz = 0;
    // include/map_local.h:201-213
    PointF subbox_id2xyz_glb(const Vec3I &origin, int idx) const {
        const Vec3d c = subbox_id2xyz_glb_vec(origin, idx);
        return PointF{(float)c[0], (float)c[1], (float)c[2]};
    }
    Vec3d subbox_id2xyz_glb_vec(const Vec3I &origin, int idx) const {
        const int n = subbox_nxyz, cz = idx / (n * n), cy = (idx - cz * n * n) / n, cx = idx - cz * n * n - cy * n;
        return Vec3d{{origin[0] * map_dxyz_obv_glb + cx * map_dxyz_obv_sub + map_dxyz_obv_sub_half,
                      origin[1] * map_dxyz_obv_glb + cy * map_dxyz_obv_sub + map_dxyz_obv_sub_half,
                      origin[2] * map_dxyz_obv_glb + cz * map_dxyz_obv_sub + map_dxyz_obv_sub_half}};
    }
};

class mlmap {
  public:
    // include/mlmap.h:109-114
    enum { FREE = 1, OCCUPIED = 0, UNKNOWN = -1 };
    bool has_data = false;    // mlmap.h:115
    bool map_updated = false; // mlmap.h:116

    mlmap() = default;
    mlmap(const mlmap &) = delete;
    mlmap &operator=(const mlmap &) = delete;
    ~mlmap() {
        if (h_) mlm_destroy(h_);
    }

    // replaces init_map(ros::NodeHandle&) (src/mlmap.cpp:3-149): the caller reads the YAML keys into mlm_config
    void init_map(const mlm_config &cfg, int device = 0, const mlm_limits *limits = nullptr) {
        if (h_) mlm_destroy(h_);
        h_ = nullptr;
        cfg_ = cfg;
        const int rc = mlm_create(&cfg, limits, device, &h_);
        if (rc != MLM_OK) {
            std::string msg = h_ ? mlm_last_error(h_) : "";
            if (h_) mlm_destroy(h_);
            h_ = nullptr;
            throw std::runtime_error("mlm_create failed (" + std::to_string(rc) + "): " + msg);
        }
        width_ = height_ = 0;
    }

    // What depth_odom_input_callback hands to project_depth()/update_map() (src/mlmap.cpp:484,494,504-507):
    // the 16UC1 depth image and the compensated pose T_wb = (q_wb (w,x,y,z), t_wb).
    void set_depth_image(const uint16_t *img, int width, int height, int row_stride = 0) {
        img_ = img;
        width_ = width;
        height_ = height;
        stride_ = row_stride ? row_stride : width;
        has_data = true;
    }
    void set_pose(const double q_wb[4], const double t_wb[3]) {
        for (int i = 0; i < 4; ++i) q_[i] = q_wb[i];
        for (int i = 0; i < 3; ++i) t_[i] = t_wb[i];
    }
    // project_depth (src/mlmap.cpp:311-349): the reference draws <= sample_cnt pixels with rand(); a host that wants
    // bit parity with it passes the same pixel list, otherwise the whole image is integrated.
    void project_depth(const std::vector<int32_t> *pixel_idx = nullptr) {
        if (pixel_idx)
            pix_ = *pixel_idx;
        else
            pix_.clear();
        sampled_ = pixel_idx != nullptr;
    }
    // update_map (src/mlmap.cpp:382-386)
    void update_map() {
        check(mlm_integrate_depth_u16(h_, img_, width_, height_, stride_, sampled_ ? pix_.data() : nullptr,
                                      (int)pix_.size(), q_, t_),
              "mlm_integrate_depth_u16");
        map_updated = true;
    }

    // src/mlmap.cpp:388-407
    template <class V3> void setFree_map_in_bound(const V3 &box_min, const V3 &box_max) {
        const double a[3] = {box_min[0], box_min[1], box_min[2]}, b[3] = {box_max[0], box_max[1], box_max[2]};
        check(mlm_set_free_in_bound(h_, a, b), "mlm_set_free_in_bound");
    }
    // include/mlmap.h:170-193
    template <class V3> int getOccupancy(const V3 &pos_w) {
        const double p[3] = {pos_w[0], pos_w[1], pos_w[2]};
        int8_t r = 0;
        check(mlm_query_occupancy(h_, p, 1, &r), "mlm_query_occupancy");
        return r;
    }
    // include/mlmap.h:142-169
    template <class V3> int getOccupancy(const V3 &pos_w, float inflate) {
        const double p[3] = {pos_w[0], pos_w[1], pos_w[2]};
        int8_t r = 0;
        check(mlm_query_occupancy_inflate(h_, p, 1, inflate, &r), "mlm_query_occupancy_inflate");
        return r;
    }
    // include/mlmap.h:195-211
    template <class V3> int getInflateOccupancy(const V3 &pos_w) {
        const double p[3] = {pos_w[0], pos_w[1], pos_w[2]};
        int8_t r = 0;
        check(mlm_query_inflate_occupancy(h_, p, 1, &r), "mlm_query_inflate_occupancy");
        return r;
    }
    // include/mlmap.h:213-225
    template <class V3> float getOdd(const V3 &pos_w) {
        const double p[3] = {pos_w[0], pos_w[1], pos_w[2]};
        float r = 0.5f;
        check(mlm_query_odds(h_, p, 1, &r), "mlm_query_odds");
        return r;
    }
    // include/mlmap.h:227-235: float getOdd(const Vec3I &glb_id, size_t subbox_id)
    template <class V3I> float getOdd(const V3I &glb_id, size_t subbox_id) {
        const int32_t g[3] = {(int32_t)glb_id[0], (int32_t)glb_id[1], (int32_t)glb_id[2]};
        const int32_t c = (int32_t)subbox_id;
        float r = 0.5f;
        check(mlm_query_odds_at(h_, g, &c, 1, &r), "mlm_query_odds_at");
        return r;
    }
    // include/mlmap.h:237-295
    template <class V3> Vec3d getOddGrad(const V3 &pos_w, size_t max_iter = 5) {
        const double p[3] = {pos_w[0], pos_w[1], pos_w[2]};
        Vec3d g{};
        check(mlm_query_odd_grad(h_, p, 1, (int)max_iter, g.v), "mlm_query_odd_grad");
        return g;
    }
    // src/mlmap.cpp:286-309 (ct_pos = vehicle position, set by the odometry callback, mlmap.cpp:485-487)
    template <class V3> void inflate_map(const V3 &ct_pos) {
        const double p[3] = {ct_pos[0], ct_pos[1], ct_pos[2]};
        check(mlm_inflate_map(h_, p), "mlm_inflate_map");
    }

    // `local_map` for visualisers: a snapshot of observed_group_map (one D2H of the block planes; waits for everything submitted)
    std::shared_ptr<local_map_view> local_map_snapshot() {
        auto lm = std::make_shared<local_map_view>();
        const int n = cfg_.subbox_n, C = n * n * n;
        lm->subbox_nxyz = n;
        lm->map_dxyz_obv_sub = cfg_.subbox_d_xyz;
        lm->map_dxyz_obv_glb = cfg_.subbox_d_xyz * n; // map_local.cpp:60
        lm->map_dxyz_obv_sub_half = cfg_.subbox_d_xyz * 0.5;
        int nb = 0;
        check(mlm_block_count(h_, &nb), "mlm_block_count");
        std::vector<int32_t> keys((size_t)nb * 3);
        std::vector<float> lo((size_t)nb * C);
        std::vector<uint8_t> occ((size_t)nb * C), infl((size_t)nb * C), col((size_t)nb);
        int m = 0;
        if (nb) {
            check(mlm_export_blocks(h_, nb, keys.data(), lo.data(), occ.data(), infl.data(), &m), "mlm_export_blocks");
            check(mlm_export_block_flags(h_, nb, col.data(), &m), "mlm_export_block_flags");
        }
        lm->observed_group_map.reserve((size_t)nb);
        for (int b = 0; b < nb; ++b) {
            auto &sb = lm->observed_group_map[Vec3I{{keys[3 * (size_t)b], keys[3 * (size_t)b + 1], keys[3 * (size_t)b + 2]}}];
            const size_t cnt = col[(size_t)b] ? 1 : (size_t)C, o = (size_t)b * C;
            sb.occupancy.assign(occ.begin() + o, occ.begin() + o + cnt);
            sb.inflate_occupancy.assign(infl.begin() + o, infl.begin() + o + cnt);
            sb.log_odds.assign(lo.begin() + o, lo.begin() + o + cnt);
        }
        int nf = 0;
        check(mlm_export_frontier(h_, 0, nullptr, &nf), "mlm_export_frontier");
        if (nf) {
            std::vector<int32_t> fr((size_t)nf * 4);
            check(mlm_export_frontier(h_, nf, fr.data(), &nf), "mlm_export_frontier");
            for (int i = 0; i < nf; ++i) {
                auto it = lm->observed_group_map.find(Vec3I{{fr[4 * (size_t)i], fr[4 * (size_t)i + 1], fr[4 * (size_t)i + 2]}});
                if (it != lm->observed_group_map.end()) it->second.frontier.insert(fr[4 * (size_t)i + 3]);
            }
        }
        return lm;
    }

    // truncated Euclidean distance field of a voxel box (mlm_export_esdf; flags MLM_ESDF_*; outputs host or device memory, NULL =
    // skipped)
    void export_esdf(const int32_t lo[3], const int32_t dims[3], int max_dist, int flags, int32_t *sqdist, float *dist = nullptr,
                     float *grad3 = nullptr) {
        check(mlm_export_esdf(h_, lo, dims, max_dist, flags, sqdist, dist, grad3), "mlm_export_esdf");
    }

    // the slab lo .. lo + dims projected onto the ground plane: occupancy grid, column statistics, plane distances
    // (mlm_export_grid2d; flags MLM_GRID_*; grid / cols / sqdist / dist host or device memory, summary host memory, NULL = skipped)
    void export_grid2d(const int32_t lo[3], const int32_t dims[3], int flags, int min_free, int z_ref, int max_dist, int8_t *grid,
                       int32_t *cols = nullptr, int32_t *sqdist = nullptr, float *dist = nullptr, int64_t summary[6] = nullptr) {
        check(mlm_export_grid2d(h_, lo, dims, flags, min_free, z_ref, max_dist, grid, cols, sqdist, dist, summary), "mlm_export_grid2d");
    }

    // cost-to-go field through the free space of a voxel box (mlm_export_reach; flags MLM_REACH_*; seeds3: n_seeds voxel index
    // triples; steps / parent host or device memory, summary host memory, NULL = skipped)
    void exportReach(const int32_t lo[3], const int32_t dims[3], const int32_t *seeds3, int n_seeds, int flags, int clearance, int max_steps,
                     int32_t *steps, uint8_t *parent = nullptr, int64_t summary[4] = nullptr) {
        check(mlm_export_reach(h_, lo, dims, seeds3, n_seeds, flags, clearance, max_steps, steps, parent, summary), "mlm_export_reach");
    }

    // clearance-weighted cost field with face / edge / corner moves through the free space of a voxel box (mlm_export_route; flags
    // MLM_ROUTE_*; connectivity 6 / 18 / 26; move_cost[3] and penalty[n_penalty] host memory; cost / parent host or device memory,
    // summary host memory, NULL = skipped)
    void exportRoute(const int32_t lo[3], const int32_t dims[3], const int32_t *seeds3, int n_seeds, int flags, int clearance, int connectivity,
                     const int32_t move_cost[3], const int32_t *penalty, int n_penalty, int max_cost, int32_t *cost, uint8_t *parent = nullptr,
                     int64_t summary[4] = nullptr) {
        check(mlm_export_route(h_, lo, dims, seeds3, n_seeds, flags, clearance, connectivity, move_cost, penalty, n_penalty, max_cost, cost, parent,
                               summary),
              "mlm_export_route");
    }
    // paths through a parent field of exportReach (kind MLM_PATH_REACH) or exportRoute (MLM_PATH_ROUTE), traced from each goal to its
    // seed and shortened to way points (mlm_query_paths; lookahead 1 .. 4096, max_moves 1 .. 2^20; parent, goals and outputs host or
    // device memory, NULL = skipped; cap rows of way3 per goal, 0 with way3 == NULL)
    void queryPaths(const int32_t lo[3], const int32_t dims[3], const uint8_t *parent, int kind, const int32_t *goals3, int n, int lookahead,
                    int max_moves, int cap, int8_t *status, int32_t *way3 = nullptr, double *length = nullptr, int64_t *table = nullptr) {
        check(mlm_query_paths(h_, lo, dims, parent, kind, goals3, n, lookahead, max_moves, cap, status, way3, length, table), "mlm_query_paths");
    }
    // one goal: its way points, goal first, seed last; empty if there is no path (goal not reached or outside the box, path longer than
    // max_moves, broken field).  length (optional): the polyline in metres.
    std::vector<Vec3I> tracePath(const int32_t lo[3], const int32_t dims[3], const uint8_t *parent, int kind, const Vec3I &goal, int lookahead,
                                 int max_moves, double *length = nullptr) {
        const int32_t g[3] = {goal[0], goal[1], goal[2]};
        int8_t st = 0;
        int64_t row[MLM_PATH_ROW] = {};
        check(mlm_query_paths(h_, lo, dims, parent, kind, g, 1, lookahead, max_moves, 0, &st, nullptr, nullptr, row), "mlm_query_paths");
        std::vector<Vec3I> out;
        if (st != 1) return out;
        std::vector<int32_t> way((size_t)row[1] * 3);
        check(mlm_query_paths(h_, lo, dims, parent, kind, g, 1, lookahead, max_moves, (int)row[1], nullptr, way.data(), length, nullptr),
              "mlm_query_paths");
        for (size_t t = 0; t < (size_t)row[1]; ++t) out.push_back(Vec3I{{way[3 * t], way[3 * t + 1], way[3 * t + 2]}});
        return out;
    }

    // connected components of a voxel set of a box with per-component statistics (mlm_export_clusters; flags MLM_CLUSTER_*;
    // connectivity 6 / 18 / 26; labels / table host or device memory, table [cap][MLM_CLUSTER_ROW], summary host memory, NULL = skipped)
    void exportClusters(const int32_t lo[3], const int32_t dims[3], int flags, int connectivity, int min_size, int32_t *labels,
                        int64_t *table = nullptr, int cap = 0, int64_t summary[6] = nullptr) {
        check(mlm_export_clusters(h_, lo, dims, flags, connectivity, min_size, labels, table, cap, summary), "mlm_export_clusters");
    }

    // exact surface mesh of the obstacle set of a box: quads over shared vertices (mlm_export_mesh; flags MLM_MESH_*; quads / face4
    // [cap_faces][4], vert3 / vert_xyz / vert_n3 [cap_verts][3], host or device memory, NULL = skipped, a cap is 0 iff all of its
    // arrays are NULL; summary host memory: [0] faces, [1] vertices whatever the caps — a call with only summary sizes the next one)
    void exportMesh(const int32_t lo[3], const int32_t dims[3], int flags, int32_t *quads, int32_t *face4, int64_t cap_faces, int32_t *vert3,
                    float *vert_xyz, int8_t *vert_n3, int64_t cap_verts, int64_t summary[MLM_MESH_ROW] = nullptr) {
        check(mlm_export_mesh(h_, lo, dims, flags, quads, face4, cap_faces, vert3, vert_xyz, vert_n3, cap_verts, summary), "mlm_export_mesh");
    }

    // exact pruned occupancy octree of a box (mlm_export_octree; depth 1..31, 16: OctoMap's key space; flags MLM_OCT_*; words / inner4 /
    // skip [cap_inner], leaf4 / leaf_class [cap_leaves], host or device memory, NULL = skipped, a cap is 0 iff all of its arrays are
    // NULL; summary host memory: [0] inner nodes, [1] leaves whatever the caps — a call with only summary sizes the next one)
    void octree(const int32_t lo[3], const int32_t dims[3], int depth, int flags, uint16_t *words, int32_t *inner4, int32_t *skip,
                int64_t cap_inner, int32_t *leaf4, int8_t *leaf_class, int64_t cap_leaves, int64_t summary[MLM_OCT_ROW] = nullptr) {
        check(mlm_export_octree(h_, lo, dims, depth, flags, words, inner4, skip, cap_inner, leaf4, leaf_class, cap_leaves, summary),
              "mlm_export_octree");
    }

    // drop — or page out — the blocks outside (MLM_CROP_INSIDE: inside) a box of block keys, in place on the device (mlm_crop_blocks;
    // flags MLM_CROP_*; keys [cap][3], log_odds / occ / infl [cap][cells], collapsed [cap], host or device memory, NULL = skipped: with
    // none of them the blocks are just dropped; summary host memory: [2] dropped blocks whatever the cap — a MLM_CROP_DRY call sizes the next one)
    void cropBlocks(const int32_t key_lo[3], const int32_t key_dims[3], int flags = MLM_CROP_OUTSIDE, int cap = 0, int32_t *keys = nullptr,
                    float *log_odds = nullptr, uint8_t *occ = nullptr, uint8_t *infl = nullptr, uint8_t *collapsed = nullptr,
                    int64_t summary[MLM_CROP_ROW] = nullptr) {
        check(mlm_crop_blocks(h_, key_lo, key_dims, flags, cap, keys, log_odds, occ, infl, collapsed, summary), "mlm_crop_blocks");
    }

    // the map resampled under a rigid transform (mlm_warp_blocks; T_sd maps the new frame to the map's; flags MLM_WARP_*; the emitted
    // blocks in ascending key order into keys [cap][3], log_odds / occ / infl [cap][cells], host or device memory, NULL = skipped;
    // summary host memory: [2] emitted blocks whatever the cap — a MLM_WARP_DRY call sizes the next one; MLM_WARP_REPLACE: the handle
    // holds the warped map afterwards)
    void warpBlocks(const double T_sd[12], const int32_t key_lo[3] = nullptr, const int32_t key_dims[3] = nullptr, int flags = 0, int cap = 0,
                    int32_t *keys = nullptr, float *log_odds = nullptr, uint8_t *occ = nullptr, uint8_t *infl = nullptr,
                    int64_t summary[MLM_WARP_ROW] = nullptr) {
        check(mlm_warp_blocks(h_, T_sd, key_lo, key_dims, flags, cap, keys, log_odds, occ, infl, summary), "mlm_warp_blocks");
    }

    // a block dump fused into the live map in place, or — MLM_FUSE_DRY — only compared with it (mlm_fuse_blocks; keys [n][3], log_odds /
    // occ / infl [n][cells] as mlm_export_blocks, cropBlocks and warpBlocks write them, host or device memory, infl may be NULL; mode
    // MLM_FUSE_ADD / MAX / TAKE / FILL; per_row [n][MLM_FUSE_COLS] host or device memory or NULL; summary host memory: [2] created
    // blocks, [7] conflicting voxels)
    void fuseBlocks(int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl = nullptr, int mode = MLM_FUSE_ADD,
                    int flags = 0, int32_t *per_row = nullptr, int64_t summary[MLM_FUSE_ROW] = nullptr) {
        check(mlm_fuse_blocks(h_, n, keys, log_odds, occ, infl, mode, flags, per_row, summary), "mlm_fuse_blocks");
    }

    // the map aged in place: the log-odds of the blocks of a key box (both NULL: of every block; MLM_AGE_OUTSIDE: of the blocks outside
    // it) scaled (MLM_AGE_SCALE, amount in [0, 1]) or stepped towards zero (MLM_AGE_STEP), small evidence forgotten (MLM_AGE_FORGET,
    // |log-odds| <= forget), the blocks left empty dropped (MLM_AGE_DROP), or — MLM_AGE_DRY — only counted (mlm_age_blocks; per_block
    // [blocks before][MLM_AGE_COLS] host or device memory or NULL; summary host memory: [2] blocks dropped, [6] forgotten voxels)
    void ageBlocks(const int32_t key_lo[3] = nullptr, const int32_t key_dims[3] = nullptr, int mode = MLM_AGE_SCALE, float amount = 1.0f,
                   float forget = 0.0f, int flags = 0, int32_t *per_block = nullptr, int64_t summary[MLM_AGE_ROW] = nullptr) {
        check(mlm_age_blocks(h_, key_lo, key_dims, mode, amount, forget, flags, per_block, summary), "mlm_age_blocks");
    }

    // what changed since the digest table prev_keys / prev_digest of an earlier call (n_prev 0: everything is new): the new table, the
    // changed and the new blocks of a key box (both NULL: of every block) in import's layout with their kind, and the keys that are
    // gone (mlm_delta_blocks; every pointer host or device memory, outputs may be NULL; MLM_DELTA_DRY only counts; summary host memory:
    // [1] table rows, [5] + [6] emitted blocks, [7] gone keys: size with a dry call first)
    void deltaBlocks(const int32_t key_lo[3], const int32_t key_dims[3], int n_prev, const int32_t *prev_keys, const uint64_t *prev_digest, int flags,
                     int cap_table, int32_t *cur_keys, uint64_t *cur_digest, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl,
                     uint8_t *kind, int cap_gone, int32_t *gone_keys, int64_t summary[MLM_DELTA_ROW]) {
        check(mlm_delta_blocks(h_, key_lo, key_dims, n_prev, prev_keys, prev_digest, flags, cap_table, cur_keys, cur_digest, cap, keys, log_odds, occ, infl, kind, cap_gone,
                               gone_keys, summary),
              "mlm_delta_blocks");
    }

    // the lossless packed stream of the live map's blocks of a key box (keys NULL; both box pointers NULL: of every block), or of n rows
    // of a dump (mlm_pack_blocks; MLM_PACK_DRY or a NULL stream only sizes: summary [1] is the stream's bytes; stream host memory or
    // 8-byte-aligned device memory) ...
    void packBlocks(const int32_t key_lo[3], const int32_t key_dims[3], int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl,
                    int flags, size_t cap_bytes, void *stream, int64_t summary[MLM_PACK_ROW]) {
        check(mlm_pack_blocks(h_, key_lo, key_dims, n, keys, log_odds, occ, infl, flags, cap_bytes, stream, summary), "mlm_pack_blocks");
    }
    // ... and a stream back into rows in import's layout (mlm_unpack_blocks; validated whole before the first store; all outputs NULL
    // sizes: summary [0] is the blocks)
    void unpackBlocks(const void *stream, size_t bytes, int flags, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl,
                      int64_t summary[MLM_PACK_ROW]) {
        check(mlm_unpack_blocks(h_, stream, bytes, flags, cap, keys, log_odds, occ, infl, summary), "mlm_unpack_blocks");
    }

    // segment casts through the voxel map (mlm_query_rays; flags MLM_RAY_*; n x 3 end points; inputs and outputs host or device
    // memory, NULL output = skipped)
    void castRays(const double *p0, const double *p1, int n, int flags, int8_t *status, int32_t *voxel3 = nullptr, double *t = nullptr,
                  int32_t *n_steps = nullptr, int32_t *n_unknown = nullptr) {
        check(mlm_query_rays(h_, p0, p1, n, flags, status, voxel3, t, n_steps, n_unknown), "mlm_query_rays");
    }
    // one segment (answered from the host mirror: no launch): true if it stops at a voxel that `flags` selects; t_hit the segment
    // parameter at which that voxel is entered (1 without a stop), voxel3 that voxel (the end voxel without a stop), n_unknown the
    // UNKNOWN voxels in front of it.  An invalid segment (not finite, longer than 32 768 voxels on an axis) throws.
    template <class V3>
    bool castRay(const V3 &p0, const V3 &p1, int flags, double *t_hit = nullptr, int32_t *voxel3 = nullptr, int32_t *n_unknown = nullptr) {
        const double a[3] = {p0[0], p0[1], p0[2]}, b[3] = {p1[0], p1[1], p1[2]};
        int8_t st = 0;
        check(mlm_query_rays(h_, a, b, 1, flags, &st, voxel3, t_hit, nullptr, n_unknown), "mlm_query_rays");
        if (st < 0) throw std::runtime_error("castRay: invalid segment");
        return st == 1;
    }

    // the depth images the map predicts for a pinhole camera (mlm_render_depth; flags MLM_RAY_*; T_ws n_poses x 12: R sensor -> world
    // row major, then the optical centre; K = fx, fy, cx, cy in host memory or NULL = the configuration's camera; outputs
    // [n_poses][height][width], depth uint16 mm as the integrate calls read it, 0 = nothing stopped the ray; table
    // [n_poses][MLM_RENDER_ROW]; T_ws and every output host or device memory, NULL output = skipped)
    void renderDepth(const double *T_ws, int n_poses, int width, int height, const double K[4], int max_depth_mm, int flags, uint16_t *depth,
                     int8_t *status = nullptr, int32_t *voxel3 = nullptr, int32_t *n_unknown = nullptr, int64_t *table = nullptr) {
        check(mlm_render_depth(h_, T_ws, n_poses, width, height, K, max_depth_mm, flags, depth, status, voxel3, n_unknown, table), "mlm_render_depth");
    }
    // one image from a body pose, as the integrate calls take it: q_wb (w, x, y, z), t_wb, composed with the configuration's T_bs
    // (a convenience outside mlm_render_depth's contract, which starts at R and o: plain double arithmetic, q_wb normalised here).
    // Compare it with the frame just received at that pose: pixels much nearer than rendered are something new.
    void renderDepthAt(const double q_wb[4], const double t_wb[3], int width, int height, int max_depth_mm, int flags, uint16_t *depth,
                       int8_t *status = nullptr) {
        double T[12];
        composeTws(q_wb, t_wb, cfg_.T_bs, T);
        renderDepth(T, 1, width, height, nullptr, max_depth_mm, flags, depth, status);
    }
    static void composeTws(const double q_wb[4], const double t_wb[3], const double T_bs[16], double T_ws[12]) {
        double n = 0.0;
        for (int i = 0; i < 4; ++i) n += q_wb[i] * q_wb[i];
        n = std::sqrt(n);
        const double w = q_wb[0] / n, x = q_wb[1] / n, y = q_wb[2] / n, z = q_wb[3] / n;
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z),     2 * (x * z + w * y),     2 * (x * y + w * z),    1 - 2 * (x * x + z * z),
                             2 * (y * z - w * x),     2 * (x * z - w * y),     2 * (y * z + w * x),     1 - 2 * (x * x + y * y)};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) T_ws[3 * r + c] = R[3 * r] * T_bs[c] + R[3 * r + 1] * T_bs[4 + c] + R[3 * r + 2] * T_bs[8 + c];
            T_ws[9 + r] = t_wb[r] + (R[3 * r] * T_bs[3] + R[3 * r + 1] * T_bs[7] + R[3 * r + 2] * T_bs[11]);
        }
    }

    // distinct-voxel gain of grouped ray fans (mlm_query_views; view k = segments view_begin[k] .. view_begin[k + 1]; flags MLM_RAY_*;
    // lo / dims the accounting box or both NULL; exclude / mark uint8 per voxel of the box; table [n_views][MLM_VIEW_ROW]; every
    // pointer host or device memory, NULL = skipped, mark or table must be given)
    void queryViews(const double *p0, const double *p1, const int32_t *view_begin, int n_views, int flags, int64_t *table,
                    const int32_t *lo = nullptr, const int32_t *dims = nullptr, const uint8_t *exclude = nullptr, uint8_t *mark = nullptr) {
        check(mlm_query_views(h_, p0, p1, view_begin, n_views, flags, lo, dims, exclude, mark, table), "mlm_query_views");
    }

    // class counts and free-space growth of axis-aligned voxel boxes (mlm_query_boxes; flags MLM_BOX_*; box6 n x 6 inclusive voxel
    // indices lo then hi; max_grow six layer counts in host memory or NULL = a pure count; lo / dims the limit window or both NULL;
    // table [n][MLM_BOX_ROW]; box6 and every output host or device memory, NULL output = skipped)
    void queryBoxes(const int32_t *box6, int n, int flags, const int32_t max_grow[6], int8_t *status, int32_t *out6 = nullptr,
                    uint8_t *closed = nullptr, int64_t *table = nullptr, const int32_t *lo = nullptr, const int32_t *dims = nullptr) {
        check(mlm_query_boxes(h_, box6, n, flags, max_grow, lo, dims, status, out6, closed, table), "mlm_query_boxes");
    }
    // one box (answered from the host mirror when its limit volume is small: no launch): the largest box the growth of
    // mlm_query_boxes reaches from [a, b]; false if [a, b] itself holds a voxel that `flags` selects.  An invalid box throws.
    bool growBox(const int32_t a[3], const int32_t b[3], int flags, const int32_t max_grow[6], int32_t out6[6], uint8_t *closed = nullptr,
                 int64_t *row = nullptr) {
        const int32_t in[6] = {a[0], a[1], a[2], b[0], b[1], b[2]};
        int8_t st = 0;
        check(mlm_query_boxes(h_, in, 1, flags, max_grow, nullptr, nullptr, &st, out6, closed, row), "mlm_query_boxes");
        if (st < 0) throw std::runtime_error("growBox: invalid box");
        return st == 1;
    }
    // exact nearest obstacle voxel of batched positions (mlm_query_nearest; flags MLM_NEAR_*, max_dist 1 .. 64 voxels; pos and outputs
    // host or device memory, NULL = skipped)
    void queryNearest(const double *pos, int n, int max_dist, int flags, int8_t *status, int32_t *voxel3 = nullptr, int32_t *delta3 = nullptr,
                      int64_t *sq = nullptr, double *dist = nullptr) {
        check(mlm_query_nearest(h_, pos, n, max_dist, flags, status, voxel3, delta3, sq, dist), "mlm_query_nearest");
    }
    // one position (answered from the host mirror while (2 max_dist + 1)^3 <= 2^18: no launch): the nearest voxel that `flags`
    // selects within max_dist voxels, its distance in metres, and optionally the vector to its centre in 1/1024 voxel; false if
    // there is none.  A position that is not finite or beyond the lattice throws.
    template <class V3> bool nearestObstacle(const V3 &pos_w, int max_dist, int flags, Vec3I &voxel, double &dist, int32_t *delta3 = nullptr) {
        const double p[3] = {pos_w[0], pos_w[1], pos_w[2]};
        int8_t st = 0;
        int32_t v[3] = {0, 0, 0};
        check(mlm_query_nearest(h_, p, 1, max_dist, flags, &st, v, delta3, nullptr, &dist), "mlm_query_nearest");
        if (st < 0) throw std::runtime_error("nearestObstacle: invalid position");
        voxel = Vec3I{{v[0], v[1], v[2]}};
        return st == 1;
    }
    // exact batched segment casts for a ball of `radius` voxels (mlm_query_sweeps; flags MLM_SWEEP_*, radius 0 .. 16; inputs and
    // outputs host or device memory, NULL = skipped)
    void querySweeps(const double *p0, const double *p1, int n, int radius, int flags, int8_t *status, int32_t *voxel3 = nullptr, double *t = nullptr,
                     int32_t *n_steps = nullptr, int32_t *n_unknown = nullptr, int32_t *hit3 = nullptr, int32_t *hit_sq = nullptr) {
        check(mlm_query_sweeps(h_, p0, p1, n, radius, flags, status, voxel3, t, n_steps, n_unknown, hit3, hit_sq), "mlm_query_sweeps");
    }
    // scan-to-map scores of candidate poses (mlm_score_poses): pts_s n_pts x 3 sensor-frame points, T_ws n_poses x 12 poses as
    // mlm_render_depth takes them, table n_poses x MLM_SCORE_ROW int64 (valid, occ, free, unknown, infl, in box, cost, zero); flags
    // MLM_SCORE_CLASSES and / or a field (lo, dims, sqdist as mlm_export_esdf wrote it; sq_cap 1 .. 2^20); every array host or device memory
    void scorePoses(const double *pts_s, int n_pts, const double *T_ws, int n_poses, int flags, int64_t *table, const int32_t *lo = nullptr,
                    const int32_t *dims = nullptr, const int32_t *sqdist = nullptr, int sq_cap = 64) {
        check(mlm_score_poses(h_, pts_s, n_pts, T_ws, n_poses, flags, lo, dims, sqdist, sq_cap, table), "mlm_score_poses");
    }
    // segment casts through a distance field (mlm_query_clearance): the walk of queryRays through sqdist over the box lo, dims (as
    // mlm_export_esdf wrote it), stopped at the first voxel with f <= sq_stop or outside the box (flags MLM_CLEAR_OUTSIDE_PASS: outside
    // voxels have f = sq_cap); per ray the stop, the minimum clearance and where, the summed cost and the near voxels; with group_begin
    // (n_groups + 1 offsets) one row of MLM_CLEAR_ROW int64 per group in table; every array host or device memory
    void queryClearance(const double *p0, const double *p1, int n, const int32_t *lo, const int32_t *dims, const int32_t *sqdist, int sq_stop,
                        int sq_cap, int flags, int8_t *status, int32_t *voxel3 = nullptr, double *t = nullptr, int32_t *n_steps = nullptr,
                        int32_t *min_sq = nullptr, int32_t *min3 = nullptr, int64_t *cost = nullptr, int32_t *n_near = nullptr,
                        const int32_t *group_begin = nullptr, int n_groups = 0, int64_t *table = nullptr) {
        check(mlm_query_clearance(h_, p0, p1, n, lo, dims, sqdist, sq_stop, sq_cap, flags, status, voxel3, t, n_steps, min_sq, min3, cost, n_near,
                                  group_begin, n_groups, table),
              "mlm_query_clearance");
    }

    // planners that query thousands of positions per cycle should use the batched entry points directly
    mlm_handle *handle() { return h_; }

  private:
    void check(int rc, const char *what) {
        if (rc != MLM_OK) throw std::runtime_error(std::string(what) + ": " + (h_ ? mlm_last_error(h_) : "no handle"));
    }
    mlm_handle *h_ = nullptr;
    mlm_config cfg_{};
    const uint16_t *img_ = nullptr;
    int width_ = 0, height_ = 0, stride_ = 0;
    double q_[4] = {1, 0, 0, 0}, t_[3] = {0, 0, 0};
    std::vector<int32_t> pix_;
    bool sampled_ = false;
};

} // namespace mlmap_hip
