/*
 * mlmap_hip.h — C ABI of the MI355X-native MLMapping map-update path (libmlmap_hip.so).
 *
 * This is the drop-in boundary for ONE path of the reference: mlmap::update_map()
 * (src/mlmap.cpp:382-386 = awareness_map_cylindrical::input_pc_pose, src/map_awareness.cpp:173-282,
 *  + local_map_cartesian::input_pc_pose_direct, src/map_local.cpp:143-237) and the query inlines
 * planners call on the result (include/mlmap.h:142-295, src/mlmap.cpp:388-407).
 *
 * The reference has no FFI: it is one C++ process.  Each entry point below names the C++ member it
 * replaces; INTEGRATION.md shows the mlmap-side stubs a maintainer would add, and
 * include/mlmap_facade.hpp is a header-only class with the reference's public names on top of this ABI.
 *
 * Conventions
 *  - every function returns 0 on success, a negative mlm_status otherwise; no exceptions cross the ABI
 *    (the reference has no error channel at all: yaml-cpp / vector::at exceptions kill the nodelet);
 *  - plain pointers and sizes only; host buffers are borrowed for the duration of the call;
 *  - one handle = one device + one HIP stream.  Every entry point takes the handle's lock, so a handle may be used
 *    from several threads (the reference serves planner queries and the depth callback from an MT nodelet,
 *    src/nodelet_map.cpp:21): calls are serialised, query_* calls observe the map as of the last integrate call
 *    that returned (in async mode they first wait for everything submitted).  mlm_last_error is per handle: read it
 *    on the thread that got the failure before that thread issues another call.  mlm_destroy must not race with
 *    other calls;
 *  - the block pool grows on demand (while it grows, the old and the new pool are resident together: about three times the old
 *    pool for a moment); after MLM_ERR_CAPACITY (device memory exhausted, a frame with more points than mlm_limits.max_points, or
 *    a pool fixed by the test knob "pool_grow" = 0) the handle stays usable: the map keeps what the failing call applied before it
 *    ran out of room, later frames integrate normally.  Blocks are created by the map-independent stage, up to three batches
 *    ahead of the stage that applies a frame: after a failed call the map may hold blocks of frames that were never applied —
 *    all 'u' / 0.0f, i.e. what the reference's allocate_ram leaves for a block nothing was integrated into — and
 *    mlm_frame_stats.n_blocks counts them;
 *  - poses are q_wb = (w,x,y,z) and t_wb of T_wb (body in world), exactly what mlmap.cpp:494 builds;
 *  - positions are world-frame doubles (Vec3 of include/common.h:22), n x 3 row-major.
 */
#ifndef MLMAP_HIP_H
#define MLMAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLM_ABI_VERSION 6 /* 6: mlm_set_host_mirror_limit */

typedef enum mlm_status {
    MLM_OK = 0,
    MLM_ERR_INVALID = -1,     /* bad argument */
    MLM_ERR_HIP = -2,         /* HIP runtime error, see mlm_last_error */
    MLM_ERR_CAPACITY = -3,    /* block pool / point capacity exceeded (map unchanged by the failing frame's tail) */
    MLM_ERR_UNSUPPORTED = -4, /* configuration outside the supported envelope */
} mlm_status;

/* mlmap::getOccupancy return values, include/mlmap.h:109-114 */
enum { MLM_FREE = 1, MLM_OCCUPIED = 0, MLM_UNKNOWN = -1 };

/* The YAML keys mlmap::init_map reads (src/mlmap.cpp:10-33,75-85); same meaning, same units.
 * Doubles that the reference casts to float (mlmap.cpp:77-81, mlmap.h:92) are cast the same way inside. */
typedef struct mlm_config {
    double am_d_rho;       /* mlmapping_am_d_Rho */
    double am_d_phi_deg;   /* mlmapping_am_d_Phi_deg */
    double am_d_z;         /* mlmapping_am_d_Z */
    int32_t am_n_rho;      /* mlmapping_am_n_Rho */
    int32_t am_n_z_below;  /* mlmapping_am_n_Z_below */
    int32_t am_n_z_over;   /* mlmapping_am_n_Z_over */
    int32_t use_raycasting;/* mlmapping_use_raycasting */
    double depth_noise_coe;/* mlmapping_depth_noise_coe */
    double subbox_d_xyz;   /* mlmapping_subbox_d_xyz */
    int32_t subbox_n;      /* mlmapping_subbox_n */
    int32_t use_exploration_frontiers; /* use_exploration_frontiers */
    double log_odds_min;   /* mlmapping_lm_log_odds_min */
    double log_odds_max;   /* mlmapping_lm_log_odds_max */
    double measurement_hit;/* mlmapping_lm_measurement_hit (stored, never used: map_local.cpp:128,159) */
    double measurement_miss;/* mlmapping_lm_measurement_miss */
    double occupied_sh;    /* mlmapping_lm_occupied_sh */
    int32_t inflate_n;     /* mlmapping_inflate_n */
    int32_t inflate_global_n; /* mlmapping_inflate_global_n */
    int32_t apply_inflate; /* mlmapping_apply_inflate */
    int32_t sample_cnt;    /* mlmapping_sample_cnt */
    double cam_cx, cam_cy, cam_fx, cam_fy; /* mlmapping_cam_* */
    double T_bs[16];       /* T_B_S, 4x4 row major (include/yamlRead.h:16-24) */
} mlm_config;

/* Sizing of the device-resident state (no reference counterpart: the reference grows std containers). */
typedef struct mlm_limits {
    int32_t max_blocks;      /* INITIAL capacity of the hashed block pool (n^3 cells each); 0 = default 65536.  The pool
                              * grows on demand (table and pool re-allocated at twice the size, blocks copied, table rebuilt
                              * on the device) like the reference's observed_group_map; MLM_ERR_CAPACITY only when the
                              * device cannot hold the larger pool (or with the test knob "pool_grow" = 0) */
    int32_t max_points;      /* largest point count of one frame; 0 = 1280*720 */
    int32_t max_batch;       /* frames integrated per launch sequence (batch entry points); 0 = 8, at most 64;
                              * every frame in flight owns a slot of scratch — ~0.06 GB at 640x480 / 0.1 m, ~0.25 GB at 1280x720 /
                              * 0.05 m for camera scenes: its lists start at what frames of max_points pixels need and are enlarged
                              * when a frame needs more (worst case 0.29 GB / 1.97 GB) — three sets of them (one being filled, one
                              * in the map-independent stage, one draining) */
    int32_t record_awareness;/* keep per-frame hit/miss lists readable via mlm_get_awareness_* (tests) */
} mlm_limits;

typedef struct mlm_handle mlm_handle;

/* Counters of the last integrated frame (the reference exposes the same facts as container sizes:
 * hit_idx_odds_hashmap.size(), miss_idx_set.size(), observed_group_map.size()). */
typedef struct mlm_frame_stats {
    int64_t n_points;      /* points fed (raw != 0) */
    int64_t n_hit_cells;   /* unique awareness hit cells  == hit_idx_odds_hashmap.size() */
    int64_t n_miss_cells;  /* unique awareness miss cells == miss_idx_set.size() */
    int64_t n_out_of_range;/* "point out range" branch, map_awareness.cpp:277 */
    int64_t n_blocks;      /* observed_group_map.size() */
    int64_t n_rehash_epochs; /* libstdc++ rehash epochs replayed for the hit container this frame (1 = none) */
    int64_t hit_bucket_count;/* emulated hit_idx_odds_hashmap.bucket_count() after this frame */
    /* device-side work counters (no reference counterpart) */
    int64_t n_multi_cells;   /* hit cells that received more than one kind of contribution (need the ordered replay) */
    int64_t n_contrib_slots; /* 16-padded contribution slots reserved for those cells */
    int64_t n_groups;        /* (wave, cell, kind) contribution groups (merged per cell in LDS before any global atomic) */
    int64_t n_rays;          /* rays walked after de-duplication */
    int64_t n_spec_replays;  /* frames so far whose Stage B had to be replayed with a rehash plan */
    int64_t n_device_atomics;   /* device-scope atomics the frame's Stage A issued, counted by the kernels (0 on the cell-table path) */
    int64_t n_sector_fallbacks; /* frames so far redone by the cell-table path (an azimuth sector overflowed its LDS tables) */
    int64_t logit_bit_exact;    /* 1: hit increments log10f(odd / (1 - odd)) carry the float bits of this host's libm (map_local.h:8);
                                 * 0: unknown libm, increments are FP64 log10 rounded once (last-place differences possible) */
    int64_t n_pool_grows;       /* times the block pool has grown so far (allocate_ram never refuses: map_local.h:215-231) */
    int64_t block_capacity;     /* blocks the pool holds now */
    int64_t n_graph_launches;   /* single frames so far submitted as one HIP-graph replay (synchronous mode: the reference's one frame
                                 * per depth callback, src/mlmap.cpp:463-507) */
    int64_t n_bin_exact_waves;  /* waves of the frame whose bins came from the reference's own FP64 sequence because a lane lay too near
                                 * a cell boundary for the certified cheap evaluation (k_bin_sectors; usually 0) */
    /* host mirror of the map (ABI 5): batches of up to a few hundred positions are answered on the host like the reference's inline
     * queries (include/mlmap.h:170-295), from a pinned copy of the block planes that is refreshed after the map changed */
    int64_t n_host_queries;     /* positions answered from the host mirror so far */
    int64_t n_mirror_refreshes; /* times the mirror was brought up to date (one kernel + one synchronisation each) */
    int64_t n_mirror_blocks;    /* blocks copied to the host by those refreshes */
    int64_t device_bytes;       /* device memory the handle holds now (map + frame slots + tables) */
    int64_t n_slot_grows;       /* times the frame slots' lists — sized by what frames need, not by the worst case — were enlarged */
} mlm_frame_stats;

/* replaces mlmap::init_map (src/mlmap.cpp:3-149), minus ROS plumbing */
int mlm_create(const mlm_config *cfg, const mlm_limits *limits_or_null, int device, mlm_handle **out);
int mlm_destroy(mlm_handle *h);
const char *mlm_last_error(mlm_handle *h);
int mlm_abi_version(void);

/* Use an externally owned HIP stream (e.g. the framework's current stream) instead of the handle's own for the
 * map-dependent stage, queries and exports.  Device inputs of the *_dev entry points may then be produced by work
 * enqueued on that stream before the call: the per-frame stage that reads them (which runs on streams of the handle)
 * is ordered behind it.  With the handle's own stream (the default) device inputs must be complete before the call. */
int mlm_set_stream(mlm_handle *h, void *hip_stream);

/* replaces mlmap::project_depth + update_map (src/mlmap.cpp:311-349,382-386).
 * img: uint16 millimetres (the 16UC1 image of mlmap.cpp:477-484), row_stride in pixels (>= width, else MLM_ERR_INVALID):
 * pixel (u, v) is img[v*row_stride + u].  An image is (height-1)*row_stride + width pixels long: the padding of a row is
 * never interpreted, and the LAST row need not be padded — no entry point reads a host image beyond its last pixel
 * (of a batch: beyond the last pixel of its last frame, (n_frames-1)*frame_stride + (height-1)*row_stride + width).
 * pixel_idx == NULL: dense — every pixel with raw != 0 in row-major order (v outer).
 * pixel_idx != NULL: exactly those pixels (v*width+u) in list order, raw == 0 skipped — lets a host reproduce
 * the reference's rand() sampler (mlmap.cpp:322-327) outside and keep parity. */
int mlm_integrate_depth_u16(mlm_handle *h, const uint16_t *img_host, int width, int height, int row_stride,
                            const int32_t *pixel_idx, int n_idx, const double q_wb[4], const double t_wb[3]);
/* same with the image already resident in device memory (HBM) */
int mlm_integrate_depth_u16_dev(mlm_handle *h, const uint16_t *img_dev, int width, int height, int row_stride,
                                const int32_t *pixel_idx_dev, int n_idx, const double q_wb[4],
                                const double t_wb[3]);
/* K frames of one stream, device resident, frame k at img_dev + k*frame_stride (in pixels); poses 4K / 3K doubles.
 * Frames are integrated in order (the update is order dependent). */
int mlm_integrate_depth_batch_dev(mlm_handle *h, const uint16_t *img_dev, int n_frames, size_t frame_stride,
                                  int width, int height, int row_stride, const double *q_wb, const double *t_wb);
/* same with host-resident frames (frame k at img_host + k*frame_stride); uploads overlap with compute */
int mlm_integrate_depth_batch(mlm_handle *h, const uint16_t *img_host, int n_frames, size_t frame_stride, int width,
                              int height, int row_stride, const double *q_wb, const double *t_wb);
/* replaces the body of mlmap::depth_odom_input_callback (src/mlmap.cpp:463-532) for a ROS-free host: depth is the
 * sensor_msgs/Image payload (encoding 32FC1 metres -> converted x1000 to 16UC1 like cv::Mat::convertTo, mlmap.cpp:480-483:
 * the dense path on the device, the sampler's few pixels on the host with the same float arithmetic; or
 * 16UC1 millimetres), odom_* / imu_w the nav_msgs/Odometry pose+twist and sensor_msgs/Imu angular velocity, stamps in
 * seconds; the pose is forwarded to the image stamp by the reference's linear model (mlmap.cpp:485-498).
 * sampled != 0: project_depth's rand() sampler (<= sample_cnt pixels, glibc rand(), v first, mlmap.cpp:322-327);
 * 0: dense.  T_wb_out (optional): compensated pose, q (w,x,y,z) then t. */
int mlm_integrate_callback(mlm_handle *h, const void *depth_host, int is_f32, int width, int height, double t_img,
                           const double odom_p[3], const double odom_q[4], const double odom_v[3], double t_odom,
                           const double imu_w[3], double t_imu, double camera2odom_latency, int sampled,
                           double T_wb_out[7]);
/* replaces awareness_map_cylindrical::input_pc_pose(PC_s, T_wb) + input_pc_pose_direct on an explicit
 * sensor-frame point list (include/map_awareness.h:74) */
int mlm_integrate_points(mlm_handle *h, const double *xyz_s_host, int n, const double q_wb[4],
                         const double t_wb[3]);

/* queries: include/mlmap.h:170-193 / :142-169 / :195-211 / :213-225 / :237-295 */
int mlm_query_occupancy(mlm_handle *h, const double *pos, int n, int8_t *out);
int mlm_query_occupancy_inflate(mlm_handle *h, const double *pos, int n, float inflate, int8_t *out);
int mlm_query_inflate_occupancy(mlm_handle *h, const double *pos, int n, int8_t *out);
int mlm_query_odds(mlm_handle *h, const double *pos, int n, float *out);
int mlm_query_odd_grad(mlm_handle *h, const double *pos, int n, int max_iter, double *out3);
/* float mlmap::getOdd(const Vec3I &glb_id, size_t subbox_id), include/mlmap.h:227-235: glb_id n x 3 block indices,
 * subbox_id n cell ids in [0, subbox_n^3) (out of range is undefined behaviour in the reference: MLM_ERR_INVALID here) */
int mlm_query_odds_at(mlm_handle *h, const int32_t *glb_id, const int32_t *subbox_id, int n, float *out);
/* src/mlmap.cpp:388-407 */
int mlm_set_free_in_bound(mlm_handle *h, const double box_min[3], const double box_max[3]);
/* mlmap::inflate_map (src/mlmap.cpp:286-309) around vehicle position ct_pos */
int mlm_inflate_map(mlm_handle *h, const double ct_pos[3]);

/* map read-out: what visualisers get by iterating local_map->observed_group_map (rviz_vis.cpp:280-321) */
int mlm_block_count(mlm_handle *h, int *n_out);
/* keys [cap*3], log_odds [cap*cells], occ / infl [cap*cells] ('u','f','o'); any pointer may be NULL; destinations may
 * be host or device memory (the global-map merge exports straight into device tensors) */
int mlm_export_blocks(mlm_handle *h, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl,
                      int *n_out);
/* collapsed [cap]: 1 for blocks the release scan (map_local.cpp:208-232) froze — their vectors have size 1 in the
 * reference, element 0 answers queries; always 0 unless use_exploration_frontiers */
int mlm_export_block_flags(mlm_handle *h, int cap, uint8_t *collapsed, int *n_out);
/* frontier cells as (gx,gy,gz,cell id) quadruples = the /frontier cloud before centre conversion (rviz_vis.cpp:267-293) */
int mlm_export_frontier(mlm_handle *h, int cap, int32_t *keys_cell, int *n_out);
/* float xyz of inflated-'o' cell centres = PointCloud2 payload of /global_map (rviz_vis.cpp:296-327), unordered */
int mlm_export_global_map(mlm_handle *h, int cap_points, float *xyz, int *n_out);
/* float xyz of the frontier cells' centres = PointCloud2 payload of /frontier (rviz_vis.cpp:267-293,
 * subbox_id2xyz_glb include/map_local.h:201-206), unordered; empty unless use_exploration_frontiers */
int mlm_export_frontier_points(mlm_handle *h, int cap_points, float *xyz, int *n_out);
/* Dense read-out of a box of voxels (no reference counterpart; every value is what the named reference query returns).
 * Voxel index per axis: v = g*subbox_n + c (g = block key, c = cell coordinate in [0, subbox_n)); the window is
 * lo[i] <= v[i] < lo[i]+dims[i], laid out [dims[2]][dims[1]][dims[0]] (x fastest).  Centre of v per axis:
 * g*d_glb + c*d_sub + d_sub/2 (subbox_id2xyz_glb_vec, map_local.h:208-213).
 *   odds  float  getOdd(glb_id, subbox_id)            mlmap.h:227-235  (0.5f for absent blocks)
 *   occ   int8   getOccupancy(centre)                 mlmap.h:170-193  (-1 / 0 / 1)
 *   infl  int8   getInflateOccupancy(centre)          mlmap.h:195-211
 *   grad  double getOddGrad(centre, max_iter), x,y,z  mlmap.h:237-295
 * Any output may be NULL (channel skipped), at least one must not be; outputs may be host or device memory; returns when
 * they are written; observes the map as queries do (async mode: waits for everything submitted).  In frontier mode a
 * released block answers from element 0 like the queries (infl: UNKNOWN).  MLM_ERR_INVALID: a dims[i] < 1, more than
 * 2^31 - 1 voxels, lo[i] + dims[i] beyond int32, max_iter < 0, no output.  MLM_ERR_CAPACITY: no device memory for the
 * scratch (odds of the window plus a halo of up to 8 voxels when grad is asked for, and a staging copy of host outputs; the
 * window is processed in tiles that bound both, kept by the handle and counted in mlm_frame_stats.device_bytes). */
int mlm_export_window(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int max_iter,
                      float *odds, int8_t *occ, int8_t *infl, double *grad3);
/* Truncated Euclidean distance field of a box of voxels (no reference counterpart: the reference's l2esdfs_batch_3d is disabled
 * upstream and is not a Euclidean transform).  Voxel indices, window, layout and centres are those of mlm_export_window.
 * C = max_dist (voxels, 1..64), d = (float)subbox_d_xyz.  The obstacle predicate O(v) is the union of what `flags` selects
 * (at least one of the first three bits):
 *   MLM_ESDF_OCC      getOccupancy(centre) == OCCUPIED
 *   MLM_ESDF_INFL     getInflateOccupancy(centre) == OCCUPIED
 *   MLM_ESDF_UNKNOWN  getOccupancy(centre) == UNKNOWN
 * i.e. a function of what mlm_export_window's occ / infl channels return at v (released frontier-mode blocks, absent blocks and
 * voxels beyond the int32 range of block keys included).  D_out(v) = min(C^2, min over all voxels o of the map with O(o) of
 * |v - o|^2) (integer squared index distance over the whole map, not the window; 0 on obstacles); D_in(v) the same with the
 * predicate negated (0 off obstacles).  Per voxel, x fastest:
 *   sqdist int32   D_out off obstacles; on obstacles 0, or -D_in with MLM_ESDF_SIGNED
 *   dist   float   d * sqrtf((float)D) for the sqdist D >= 0, -(d * sqrtf((float)-D)) for D < 0
 *   grad3  float   x,y,z: (dist(v + e_a) - dist(v - e_a)) * (float)(0.5 / subbox_d_xyz), neighbours outside the box included
 * (sqrtf correctly rounded, every other operation IEEE single without contraction).  Any output may be NULL (channel
 * skipped), at least one must not be; outputs may be host or device memory; returns when they are written; observes the map as
 * queries do.  MLM_ERR_INVALID: mlm_export_window's window errors, max_dist outside [1, 64], no obstacle bit or an unknown bit
 * in flags, no output.  MLM_ERR_CAPACITY: no device memory for the scratch (a mask and two u16 (SIGNED: 2 x u16) fields of
 * the tile grown by max_dist - 1 (+1 with grad3), and a staging copy of host outputs, kept by the handle and counted in
 * mlm_frame_stats.device_bytes). */
#define MLM_ESDF_OCC 1
#define MLM_ESDF_INFL 2
#define MLM_ESDF_UNKNOWN 4
#define MLM_ESDF_SIGNED 8
int mlm_export_esdf(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int max_dist, int flags,
                    int32_t *sqdist, float *dist, float *grad3);
/* The map projected onto the ground plane: an occupancy grid of a height band, per-column statistics and the plane distance to the
 * nearest blocked cell.  (Takes the place of the reference's Local2OccupancyGrid2D, include/independent_modules/l2grid2d.{h,cpp},
 * the /occupancy_map publisher behind use_projected_2d_map: it is written against a dense array the reference no longer allocates
 * and is disabled upstream, mlmap.cpp:102-109.  The classes are those of the reference's point queries, exactly as
 * mlm_export_window returns them; everything else is defined here, in integers.)
 *   Slab: lo / dims form a window under mlm_export_window's rules and errors, and lo[2] > INT32_MIN.  The cell (x, y) of the plane
 *   stands for the column of voxels (x, y, z), lo[2] <= z < lo[2] + dims[2].  The 2-D outputs are laid out [dims[1]][dims[0]], x
 *   fastest: nav_msgs/OccupancyGrid's data order with width = dims[0], height = dims[1], resolution = subbox_d_xyz and origin
 *   lo * subbox_d_xyz.
 *   Predicate: O(v) is mlm_export_esdf's — the union of what MLM_GRID_OCC / _INFL / _UNKNOWN select on what mlm_export_window's
 *   occ / infl channels return at v (released frontier-mode blocks, absent blocks and voxels beyond the key range included); at
 *   least one of the three bits.
 *   Column counts: n_obs voxels with O, n_unk voxels with occ == UNKNOWN, n_free voxels with occ == FREE.  The sets may overlap
 *   (an unknown voxel counts in n_obs too with MLM_GRID_UNKNOWN; an inflated voxel may be FREE).
 *   grid  int8   100 if n_obs > 0; otherwise -1 if n_free < min_free; otherwise 0.  0 <= min_free <= dims[2].  With min_free == 0 and
 *                flags == MLM_GRID_OCC this is the reference's rule: 0 unless an occupied cell lies in the band, then 100
 *                (l2grid2d.cpp:46-69).
 *   cols  int32 x MLM_GRID_COL per cell; z_ref is an absolute voxel index, lo[2] <= z_ref < lo[2] + dims[2] (validated only when
 *                cols is given):
 *                  [0] n_obs   [1] n_unk   [2] n_free
 *                  [3] the smallest z with O                          (none: lo[2] + dims[2])
 *                  [4] the largest z with O                           (none: lo[2] - 1)
 *                  [5] below: the largest z <= z_ref with O           (none: lo[2] - 1)
 *                  [6] above: the smallest z >= z_ref with O          (none: lo[2] + dims[2])
 *                  [7] UNKNOWN voxels with below < z < above
 *                so above - below - 1 is the obstacle-free height around z_ref: the whole slab if the column has no obstacle, -1
 *                if z_ref itself is one.
 *   Distance: P(x, y), defined for every cell of the plane and not only the box, is grid == 100 of that column over the same z
 *   range, or grid != 0 with MLM_GRID_DIST_UNOBSERVED.  C = max_dist, 1 <= C <= 64, required when sqdist or dist is given and
 *   ignored otherwise.
 *   sqdist int32  D = min(C^2, min over the cells (x', y') with P of (x - x')^2 + (y - y')^2)
 *   dist   float  d * sqrtf((float)D), d = (float)subbox_d_xyz (sqrtf correctly rounded, one multiply: mlm_export_esdf's formula).
 *                 There is no signed form and no gradient.
 *   summary int64 x 6 (host memory): [0], [1], [2] the cells with grid 100, 0 and -1; [3], [4], [5] the sums of n_obs, n_unk and
 *                 n_free over the box.
 * grid, cols, sqdist and dist may each be host or device memory; any of the five outputs may be NULL, at least one must not be.
 * Every word is a count, an extremum or an exact integer transform, so it has one value whatever the schedule.  The call observes the
 * map as queries do (async mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns when the outputs
 * are written.  There is no host-mirror shortcut.  MLM_ERR_INVALID: the window errors, lo[2] == INT32_MIN, no class bit or an
 * unknown bit in flags, min_free outside [0, dims[2]], z_ref outside the slab with cols, max_dist outside [1, 64] with sqdist /
 * dist, no output.  MLM_ERR_CAPACITY: no device memory for the scratch — 256 bytes of counters and, with sqdist / dist, a mask byte
 * and two u16 fields per cell of the tile grown by max_dist - 1 per side (the plane is processed in tiles of whole rows, a grown
 * tile has at most 2^24 cells: 80 MB), sharing mlm_export_esdf's buffer — or for the staging of host outputs (at most 41 bytes x
 * 2^20 cells, each channel rounded up to 256 bytes, sharing mlm_export_window's buffer); both are kept by the handle and counted in
 * mlm_frame_stats.device_bytes.  The handle stays usable after either error. */
#define MLM_GRID_OCC 1              /* same bits and meaning as MLM_ESDF_OCC / _INFL / _UNKNOWN */
#define MLM_GRID_INFL 2
#define MLM_GRID_UNKNOWN 4
#define MLM_GRID_DIST_UNOBSERVED 16 /* cells with grid == -1 are obstacles of the distance field too */
#define MLM_GRID_COL 8              /* int32 per column row */
int mlm_export_grid2d(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, int min_free, int z_ref,
                      int max_dist, int8_t *grid, int32_t *cols, int32_t *sqdist, float *dist, int64_t summary[6]);
/* Batched segment casts through the voxel map (no reference counterpart: the reference has no segment query; the classes a ray
 * meets are those of its point queries, the path is defined here, in integers).  Segment i runs from p0[i] to p1[i] (n x 3 world
 * positions).  d = subbox_d_xyz, voxel indices are those of mlm_export_window.
 *   Lattice: a coordinate x becomes q = floor((x / d) * 1024.0) in IEEE double.  A ray is INVALID (status -1, voxel3 0,0,0, t 0.0,
 *   counts 0) if one of its six q is not finite or |q| >= 2^40, or if |Q1 - Q0| > 2^25 on an axis (32 768 voxels).  Otherwise
 *   D = Q1 - Q0, start voxel v = Q0 >> 10, end voxel e = Q1 >> 10 (floor), N = sum over the axes of |e - v|.  The start voxel is
 *   floor(x / d) per axis, the voxel whose mlm_export_window entry is read: at the few positions where the reference's two
 *   divisions in get_global_idx / get_subbox_id disagree (the id-0 quirk) that is not the cell getOccupancy(pos) reads.
 *   Steps: per axis with D != 0, s = sign(D) and m = s > 0 ? ((v + 1) << 10) - Q0 : Q0 - (v << 10), so m / |D| is the segment
 *   parameter at which the ray leaves the current voxel along that axis.  Exactly N times: among the axes with v != e take the
 *   one with the smallest m / |D| (compared by cross-multiplication in 64 bits), ties to the lowest axis (x before y before z);
 *   (m, |D|) of that axis is the entry parameter of the next voxel; v += s, m += 1024.  The path is 6-connected, has N + 1 voxels,
 *   ends at e, and every voxel of it touches the closed segment: a ray through an exact edge or corner also visits the voxels it
 *   grazes (conservative for collision checks, and deterministic).
 *   Predicate: O(v) is the union of what `flags` selects — MLM_RAY_OCC getOccupancy(centre) == OCCUPIED, MLM_RAY_INFL
 *   getInflateOccupancy(centre) == OCCUPIED, MLM_RAY_UNKNOWN getOccupancy(centre) == UNKNOWN — i.e. mlm_export_esdf's predicate on
 *   what mlm_export_window's occ / infl channels return at v (released frontier-mode blocks, absent blocks and voxels beyond the
 *   key range included).  flags == 0: nothing stops the ray (a pure count).  Voxels are tested in path order from the start voxel
 *   (path index 0).  Per ray:
 *                          stopped at path index k (first voxel with O)          no voxel with O
 *     status    int8       1                                                      0
 *     voxel3    int32 x 3  that voxel                                             e
 *     t         double     (double)m / (double)|D| of the step that entered it;   1.0
 *                          0.0 for k = 0
 *     n_steps   int32      k                                                      N + 1
 *     n_unknown int32      voxels with occ == UNKNOWN among path indices 0..k-1   the same over the whole path
 *   p0 + t (p1 - p0) is where the segment enters the stopping voxel (up to the 1/1024-voxel lattice); n_unknown is the exploration
 *   gain of the ray.
 * Inputs and outputs may be host or device memory, each pointer on its own; any output may be NULL, at least one must not be.  The
 * call returns when the outputs are written, observes the map as queries do (async mode: waits for everything submitted) and runs
 * on the stream of mlm_set_stream.  Small batches in host memory are answered from the host mirror like small query batches (same
 * answers).  MLM_ERR_INVALID: n < 0, a NULL input with n > 0, an unknown flag bit, no output; n == 0 is MLM_OK.  MLM_ERR_CAPACITY:
 * no device memory for the staging of host inputs / outputs (at most 77 bytes x 2^20 rays, kept by the handle and counted in
 * mlm_frame_stats.device_bytes; larger batches run in chunks). */
#define MLM_RAY_OCC 1 /* same bits and same meaning as MLM_ESDF_OCC / _INFL / _UNKNOWN */
#define MLM_RAY_INFL 2
#define MLM_RAY_UNKNOWN 4
int mlm_query_rays(mlm_handle *h, const double *p0, const double *p1, int n, int flags, int8_t *status, int32_t *voxel3, double *t,
                   int32_t *n_steps, int32_t *n_unknown);
/* Expected depth images of the map: what should a pinhole camera see from this pose?  (No reference counterpart: the reference
 * projects depth images into the map, project_depth, mlmap.cpp:338-349, and has no inverse.)  Per pose and pixel one segment is
 * made on the device — its end points never exist in memory — and walked exactly as mlm_query_rays walks it.
 *   Poses: T_ws is [n_poses][12] doubles, per pose R (3 x 3, sensor to world, row major) followed by the optical centre o in the
 *   world: the caller composes T_wb * T_bs (the Python binding and the facade have a convenience for it).  K = fx, fy, cx, cy in
 *   host memory, NULL: the handle's cam_fx, cam_fy, cam_cx, cam_cy.  Z = (double)max_depth_mm / 1000.0.
 *   The segment of pixel (u, v), integers as in project_depth (0 <= u < width, 0 <= v < height): xs = (((double)u - cx) * Z) / fx,
 *   ys = (((double)v - cy) * Z) / fy, zs = Z; p0 = o; p1[a] = ((R[a][0] * xs + R[a][1] * ys) + R[a][2] * zs) + o[a] — every
 *   operation one IEEE double operation in that order, nothing fused.  It ends on the plane of z-depth Z in front of the camera.
 *   The walk: lattice, validity, path, tie rule, predicate and classes are mlm_query_rays'; flags are the MLM_RAY_* bits with their
 *   meaning there (0: nothing stops a ray).  A non-finite entry of T_ws is no error: the pixels of that pose are invalid rays, as
 *   are all pixels when Z / subbox_d_xyz exceeds 32 768 voxels on an axis.
 *   Outputs, [n_poses][height][width] with u fastest:
 *     depth     uint16     millimetres of z-depth, the 16UC1 format the integrate calls read.  status 1: z = t * (double)max_depth_mm
 *                          (one multiply), depth = min(65535, max(1, (long long)floor(z + 0.5))); status 0 or -1: 0.  So depth == 0
 *                          iff nothing stopped the ray: a sensor's "no return", which the integrate calls skip.
 *     status    int8       \
 *     voxel3    int32 x 3   > mlm_query_rays' values for that segment
 *     n_unknown int32      /
 *   table (optional): int64 [n_poses][MLM_RENDER_ROW]: [0] pixels with status 1, [1] pixels with status 0, [2] invalid pixels,
 *   [3] the sum of n_unknown over the pose.  Sums of integers: one value whatever the schedule.
 * T_ws and every output may be host or device memory, each pointer on its own; any output may be NULL, at least one must not be.
 * The call returns when the outputs are written, observes the map as queries do (async mode: waits for everything submitted) and
 * runs on the stream of mlm_set_stream.  There is no host-mirror shortcut: every call is a kernel launch (an image is thousands of
 * rays).  MLM_ERR_INVALID: n_poses < 0, T_ws NULL with n_poses > 0, width or height outside 1..8192, more than 2^31 - 1 pixels in
 * all, fx or fy not finite or not > 0, cx or cy not finite, max_depth_mm outside 1..65535, an unknown flag bit, no output;
 * n_poses == 0 is MLM_OK.  MLM_ERR_CAPACITY: no device memory for the staging of what lies in host memory: 96 bytes per pose
 * for T_ws and 32 bytes per pose for table (the whole call), and for the per-pixel outputs at most 19 bytes (2 depth, 1 status,
 * 12 voxel3, 4 n_unknown) x the pixels of one chunk — the call runs in chunks of whole rows of tiles, at most 2^20 pixels each;
 * a call of at most 2^20 pixels is one chunk —, each part rounded up to 256 bytes; the staging is kept by the handle (it shares
 * mlm_query_rays' buffer) and counted in mlm_frame_stats.device_bytes.  The handle stays usable after either error. */
#define MLM_RENDER_ROW 4
int mlm_render_depth(mlm_handle *h, const double *T_ws, int n_poses, int width, int height, const double K[4], int max_depth_mm,
                     int flags, uint16_t *depth, int8_t *status, int32_t *voxel3, int32_t *n_unknown, int64_t *table);
/* Distinct-voxel gain of grouped ray fans: from which candidate pose is the most unknown space seen?  (No reference counterpart:
 * the reference has no view query.)  The sum of mlm_query_rays' n_unknown over a fan is not that number: the rays of a fan share
 * voxels near the origin (a 64 x 48 fan of 4 m at d = 0.1 visits each of its voxels 3.5 times on average).  This call counts sets.
 *   Views and rays: view k is the group of segments view_begin[k] <= i < view_begin[k + 1] of p0 / p1 (n x 3 world positions,
 *   n = view_begin[n_views]); view_begin[0] >= 0, non-decreasing.  The rays of a view need not share an origin (the swept volume
 *   of a trajectory is a view).  Each ray is walked exactly as mlm_query_rays walks it with the same `flags` (MLM_RAY_OCC | _INFL |
 *   _UNKNOWN, 0: nothing stops it): lattice, path, tie rule, stop predicate and validity are the ones stated there.  For ray i with
 *   mlm_query_rays' (status, n_steps = k_i): its traversed voxels are path indices 0 .. k_i - 1 (the whole path without a stop), its
 *   stop voxel is path index k_i if status == 1; an invalid ray contributes no voxel.
 *   Box: lo and dims are both NULL (B = all voxels) or both given (B = the window lo <= v < lo + dims, mlm_export_window's rules and
 *   errors).  Rays walk and stop outside B as usual; only the accounting is restricted to B.
 *   Sets: A_k = the union of the traversed voxels of view k, cut to B; S_k = the union of its stop voxels, cut to B.  The stop
 *   predicate is a function of the voxel alone, so A_k and S_k are disjoint.
 *   exclude (optional, needs the box): uint8 per voxel of the box, window layout ([dims[2]][dims[1]][dims[0]], x fastest);
 *   E = the voxels with a non-zero byte, counted in none of the words [0..3].
 *   mark (optional, needs the box): same layout; for every view mark[v] |= 1 for v in A_k and mark[v] |= 2 for v in S_k,
 *   independent of exclude; all other bytes are left as they were.  An OR over views, so schedule-independent.
 *   table (optional): int64 [n_views][MLM_VIEW_ROW]:
 *     [0] |A_k \ E|                                   [4] rays with status 1
 *     [1] of those, voxels whose occ class is UNKNOWN   [5] invalid rays
 *         (the gain of the view)                        [6] sum of n_steps over the valid rays (visits with multiplicity,
 *     [2] of those, voxels whose occ class is FREE          regardless of B and E); [6] / ([0] + [3]) is the overlap factor
 *     [3] |S_k \ E| (visible surface voxels)           [7] 0, or 1 if the view was refused
 *   Classes are what mlm_export_window's occ / infl channels return (released blocks, absent blocks and voxels beyond the key
 *   range included), as for mlm_query_rays.
 *   Refused views: the bounding box of a view is the box spanned by the start and end voxels of its valid rays, cut to B (the set
 *   is kept as one bit per voxel of it).  If it holds more than 2^31 - 1 voxels the view is refused: words [0..6] are 0, [7] is 1,
 *   nothing is marked for it, and the call still returns MLM_OK.
 * Greedy view selection: score all candidates, mark the winner into a zeroed box, pass that box as exclude and score again.
 * Each pointer on its own may be host or device memory; at least one of mark / table must be given.  Every value is a set
 * cardinality or a sum, so it has exactly one value whatever the schedule.  The call observes the map as queries do (async mode:
 * waits for everything submitted), runs on the stream of mlm_set_stream and returns when the outputs are written.
 * MLM_ERR_INVALID: n_views < 0, view_begin NULL, negative at [0] or decreasing, p0 / p1 NULL with rays, an unknown flag bit, lo
 * without dims, the window errors, exclude or mark without a box, mark == exclude, no output; n_views == 0 is MLM_OK.
 * MLM_ERR_CAPACITY: no device memory for the scratch (bounding boxes, work lists, the bitsets of views too large for on-chip
 * memory: at most 256 MiB at a time, which is also the most one view can need) or the staging of host inputs / outputs (rays in chunks of views
 * of about 2^20 rays — a longer view whole —, a host exclude / mark the whole box), kept by the handle and counted in
 * mlm_frame_stats.device_bytes.  The handle stays usable after either error. */
#define MLM_VIEW_ROW 8
int mlm_query_views(mlm_handle *h, const double *p0, const double *p1, const int32_t *view_begin, int n_views, int flags,
                    const int32_t lo[3], const int32_t dims[3], const uint8_t *exclude, uint8_t *mark, int64_t *table);
/* Class counts and exact free-space growth of axis-aligned voxel boxes: is this box free, how much of it is unknown, and how far
 * can it be grown before it touches an obstacle?  (No reference counterpart: the reference has no volume query; the classes are
 * those of its point queries, the growth is defined here, in integers, with exactly one answer.)  Voxel indices and classes are
 * those of mlm_export_window (released frontier-mode blocks, absent blocks and voxels beyond the key range, which are UNKNOWN,
 * included).
 *   Faces: 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z (the parent codes of mlm_export_reach).
 *   Items: item i is the box B0 = [a, b], box6[6i .. 6i+2] = a, box6[6i+3 .. 6i+5] = b, inclusive voxel indices.  It is INVALID if
 *   a > b on an axis, b - a >= 2^15 on an axis, or a limit window is given and B0 does not lie inside it: status -1, out6 = the
 *   six input words, closed 0, a table row of zeros.
 *   Predicate: O(v) is the union of what `flags` selects (MLM_BOX_OCC getOccupancy(centre) == OCCUPIED, MLM_BOX_INFL
 *   getInflateOccupancy(centre) == OCCUPIED, MLM_BOX_UNKNOWN getOccupancy(centre) == UNKNOWN), exactly as in mlm_query_rays;
 *   flags == 0: nothing blocks.
 *   Limits: max_grow[c] in 0 .. 4096 (host memory) is the most layers face c may move outward from B0; NULL: all zero, the call is
 *   a pure count of B0.  lo / dims are both NULL or both given: W is then a window under mlm_export_window's rules and errors, and
 *   the box never leaves W.  A face whose next layer would leave W, exceed max_grow[c] or leave int32 is closed by limit.
 *   Blocked start: if B0 holds a voxel with O: status 0, out6 = B0, closed 0, no growth; table word [2] counts the O voxels of B0
 *   in full.
 *   Growth: otherwise status 1, all six faces start open.  Rounds are repeated until no face is open; a round visits the faces in
 *   order c = 0 .. 5 and skips closed ones: (1) a face at a limit is closed by limit; (2) otherwise its slab is the one-voxel layer
 *   adjacent to the current box on face c, spanning the box's current extent on the other two axes (what faces earlier in the same
 *   round have added included); (3) if a slab voxel has O the face is closed by obstacle; (4) otherwise the box absorbs the slab.
 *   Closing is permanent (exact: the slabs of a face only ever grow, so a blocked slab stays blocked).
 *   Per item:
 *     status  int8       1 grown, 0 blocked start, -1 invalid
 *     out6    int32 x 6  the final box, lo then hi, inclusive
 *     closed  uint8      bit c set iff face c was closed by an obstacle (clear: closed by limit)
 *     table   int64 x MLM_BOX_ROW  [0] voxels of the final box  [1] of those, voxels whose occ class is UNKNOWN
 *                                  [2] of those, voxels with O (non-zero only at status 0)  [3] slabs absorbed
 *   A slab has fewer than 40 960^2 < 2^31 voxels, a box fewer than 2^48.  Every word is a function of the map and the arguments
 *   alone.
 * Any output may be NULL, at least one must not be; box6 and each output on its own may be host or device memory.  The call
 * observes the map as queries do (async mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns
 * when the outputs are written.  A batch in host memory of at most 64 boxes (8 while the host mirror needs a refresh; a quarter
 * of the mirror's batch limits) whose limit volumes — B0 plus max_grow per face, cut to W — sum to at most 16 384 voxels is
 * answered from the host mirror without a launch (same answers); everything else, and every batch after
 * mlm_set_host_mirror_limit(h, 0), runs as a kernel.  MLM_ERR_INVALID: n < 0, box6 NULL with n > 0, an unknown flag bit, a max_grow
 * entry outside [0, 4096], lo without dims or the reverse, the window errors, no output; n == 0 is MLM_OK.  MLM_ERR_CAPACITY: no
 * device memory for the staging of host inputs / outputs (at most 82 bytes x 2^18 boxes, kept by the handle and counted in
 * mlm_frame_stats.device_bytes; larger batches run in chunks).  The handle stays usable after either error. */
#define MLM_BOX_OCC 1 /* same bits and same meaning as MLM_RAY_OCC / _INFL / _UNKNOWN */
#define MLM_BOX_INFL 2
#define MLM_BOX_UNKNOWN 4
#define MLM_BOX_ROW 4
int mlm_query_boxes(mlm_handle *h, const int32_t *box6, int n, int flags, const int32_t max_grow[6],
                    const int32_t lo[3], const int32_t dims[3],
                    int8_t *status, int32_t *out6, uint8_t *closed, int64_t *table);
/* Exact nearest obstacle voxel of batched points: for each position the obstacle voxel closest to it and the vector to that voxel's
 * centre, with a sub-voxel part — the {point, obstacle} pair gradient-based trajectory optimisers push away from.  (No reference
 * counterpart: the reference has no such query; the classes are those of its point queries, the metric and the tie rule are defined
 * here, in integers, with exactly one answer.)  Voxel indices and classes are those of mlm_export_window.
 *   Lattice: position i is pos[3i .. 3i+2], world frame.  Per axis Q = floor((x / d) * 1024.0) (IEEE double, d = subbox_d_xyz):
 *   mlm_query_rays' lattice, 1024 units per voxel.  The point is INVALID if a Q is not finite or |Q| >= 2^40: status -1, voxel3
 *   0,0,0, delta3 0,0,0, sq MLM_NEAR_NONE, dist -1.0.  v = Q >> 10 (floor) is the point's voxel; |v| <= 2^30, so no index below
 *   leaves int32.
 *   Predicate: O(o) is the union of what `flags` selects (MLM_NEAR_OCC getOccupancy(centre) == OCCUPIED, MLM_NEAR_INFL
 *   getInflateOccupancy(centre) == OCCUPIED, MLM_NEAR_UNKNOWN getOccupancy(centre) == UNKNOWN), exactly as in mlm_query_rays
 *   (released frontier-mode blocks, absent blocks and voxels beyond the key range, which are UNKNOWN, included); at least one of the
 *   three bits must be set.
 *   Metric: C = max_dist, 1 .. 64 voxels.  For a voxel o, delta_a(o) = 1024 * o_a + 512 - Q_a is the vector from the point to the
 *   centre of o in 1/1024 voxel, E(o) = sum over the axes of delta_a^2 (int64, below 2^34).  The candidates are the voxels of the
 *   whole map with O(o) and E(o) <= (1024 * C)^2: a ball, not a cube; every candidate has |o_a - v_a| <= C.
 *   Answer: the candidate with the smallest key = E * 2^24 + (o_z - v_z + 64) * 2^16 + (o_y - v_y + 64) * 2^8 + (o_x - v_x + 64):
 *   the smallest E, ties to the smallest z, then y, then x.
 *   Per point:                        candidate found                         no candidate
 *     status  int8                    1                                       0
 *     voxel3  int32 x 3               o                                       v
 *     delta3  int32 x 3               delta(o)                                0,0,0
 *     sq      int64                   E(o)                                    MLM_NEAR_NONE
 *     dist    double                  ((double)(float)d * sqrt((double)E)) / 1024.0   -1.0
 *   dist is three IEEE double operations in that order (sqrt correctly rounded, nothing fused); -delta3 / |delta3| is the direction
 *   that gains clearance fastest.  For a point on a voxel centre sq == 2^20 * |v - o|^2, mlm_export_esdf's sqdist wherever
 *   sqdist < C^2.  Every word is a function of the map and the arguments alone.
 * Any output may be NULL, at least one must not be; pos and each output on its own may be host or device memory.  The call observes
 * the map as queries do (async mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns when the
 * outputs are written.  A batch in host memory of at most 64 points (8 while the host mirror needs a refresh: mlm_query_boxes' rule)
 * with n * (2C + 1)^3 <= 2^18 is answered from the host mirror without a launch (same answers); everything else, and every batch
 * after mlm_set_host_mirror_limit(h, 0), runs as a kernel.  MLM_ERR_INVALID: n < 0, pos NULL with n > 0, no class bit set or an
 * unknown flag bit, max_dist outside [1, 64], no output; n == 0 is MLM_OK.  MLM_ERR_CAPACITY: no device memory for the staging of
 * host inputs / outputs (at most 65 bytes x 2^18 points, each part rounded up to 256 bytes, in the buffer mlm_query_rays stages in,
 * kept by the handle and counted in mlm_frame_stats.device_bytes; larger batches run in chunks).  The handle stays usable after
 * either error. */
#define MLM_NEAR_OCC 1 /* same bits and same meaning as MLM_RAY_OCC / _INFL / _UNKNOWN */
#define MLM_NEAR_INFL 2
#define MLM_NEAR_UNKNOWN 4
#define MLM_NEAR_NONE (-1) /* sq of a point with no obstacle in range */
int mlm_query_nearest(mlm_handle *h, const double *pos, int n, int max_dist, int flags,
                      int8_t *status, int32_t *voxel3, int32_t *delta3, int64_t *sq, double *dist);
/* Exact batched segment casts for a ball of robot radius: "is the piece from a to b free for a vehicle of radius r, and if not, where
 * does it stop and which obstacle voxel is responsible?"  (No reference counterpart: the reference has no segment query; the classes
 * are those of its point queries, the stop rule is defined here, in integers, with exactly one answer.)  Segment i runs from
 * p0[3i .. 3i+2] to p1[3i .. 3i+2].  The lattice, the validity rule, the path u_0 .. u_N, the tie rule of the walk and the classes
 * are mlm_query_rays'.
 *   Stop predicate: O(o) is the union of what `flags` selects (MLM_SWEEP_OCC / _INFL / _UNKNOWN, as MLM_RAY_*; flags == 0: nothing
 *   stops a ray).  r = radius, 0 .. MLM_SWEEP_MAX_RADIUS voxels.  BLOCKED_r(v) holds iff some voxel o of the whole map has O(o) and
 *   |o - v|^2 <= r^2 (integer squared index distance) — mlm_export_reach's BLOCKED at clearance r, so an edge checked here and a field
 *   of mlm_export_reach / mlm_export_route agree voxel for voxel about "free for radius r".  The sweep stops at the smallest path
 *   index k with BLOCKED_r(u_k).
 *   Per ray:                stopped at k                                        not stopped     invalid
 *     status     int8       1                                                   0               -1
 *     voxel3     int32 x 3  u_k (the ball's centre voxel)                       e               0,0,0
 *     t          double     (double)m / (double)|D| of the step that entered    1.0             0.0
 *                           u_k; 0.0 for k = 0
 *     n_steps    int32      k                                                   N + 1           0
 *     n_unknown  int32      centre-path voxels 0 .. k-1 whose occ is UNKNOWN    over the path   0
 *     hit3       int32 x 3  the o with O(o), |o - u_k|^2 <= r^2 and the         e               0,0,0
 *                           smallest (|o - u_k|^2, o_z, o_y, o_x)
 *     hit_sq     int32      |hit3 - u_k|^2                                      MLM_SWEEP_NONE  MLM_SWEEP_NONE
 *   (hit3's tie rule is mlm_query_nearest's.)  With radius 0 status, voxel3, t, n_steps and n_unknown are mlm_query_rays' bytes, and at
 *   a stop hit3 == voxel3, hit_sq == 0.  For a stopped ray mlm_export_esdf's sqdist at max_dist r + 1 equals hit_sq at u_k and is
 *   greater than r^2 at u_0 .. u_{k-1}.  Every word is a function of the map and the arguments alone.
 * Any output may be NULL, at least one must not be; p0, p1 and each output on its own may be host or device memory.  The call observes
 * the map as queries do (async mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns when the
 * outputs are written.  A batch in host memory of at most 64 rays (8 while the host mirror needs a refresh) whose valid rays' sum of
 * (2r + 1)^3 + N * L(r) is at most 2^18 — L(r) the number of (p, q) with p^2 + q^2 <= r^2 — is answered from the host mirror without a
 * launch (same answers); everything else, and every batch after mlm_set_host_mirror_limit(h, 0), runs as a kernel.  MLM_ERR_INVALID:
 * n < 0, a NULL input with n > 0, an unknown flag bit, radius outside [0, 16], no output; n == 0 is MLM_OK.  MLM_ERR_CAPACITY: no
 * device memory for the staging of host inputs / outputs (at most 93 bytes x 2^18 rays, each part rounded up to 256 bytes, in the
 * buffer mlm_query_rays stages in, kept by the handle and counted in mlm_frame_stats.device_bytes; larger batches run in chunks).
 * The handle stays usable after either error. */
#define MLM_SWEEP_OCC 1 /* same bits and same meaning as MLM_RAY_OCC / _INFL / _UNKNOWN */
#define MLM_SWEEP_INFL 2
#define MLM_SWEEP_UNKNOWN 4
#define MLM_SWEEP_MAX_RADIUS 16
#define MLM_SWEEP_NONE (-1) /* hit_sq of a ray that was not stopped */
int mlm_query_sweeps(mlm_handle *h, const double *p0, const double *p1, int n, int radius, int flags,
                     int8_t *status, int32_t *voxel3, double *t, int32_t *n_steps, int32_t *n_unknown,
                     int32_t *hit3, int32_t *hit_sq);
/* Exact scan-to-map scores of candidate poses: for every pose, what the map says at the voxels a cloud of sensor-frame points falls
 * into under that pose — class counts and the summed cost of a distance field — the inner loop of a correlative scan matcher or a
 * particle filter.  One lookup per (pose, point), summed per pose; no ray is walked.  (No reference counterpart: the reference takes
 * T_wb from an external odometry and only compensates its latency, mlmap.cpp:485-498; the classes are those of its point queries,
 * the lattice is mlm_query_rays', the field is mlm_export_esdf's sqdist — the likelihood-field model's log-likelihood up to a scale.)
 *   Points and poses: pts_s is [n_pts][3] positions in the sensor frame (what project_depth makes of a depth image, or any cloud);
 *   T_ws is [n_poses][12] as in mlm_render_depth: R (3 x 3, sensor to world, row major), then the optical centre o.
 *   World position of point j under pose k: w_a = ((R[a][0] * s0 + R[a][1] * s1) + R[a][2] * s2) + o[a], every operation one IEEE
 *   double operation in that order, nothing fused.
 *   Lattice and voxel: per axis Q = floor((w / d) * 1024.0) (d = subbox_d_xyz): mlm_query_rays' lattice.  The pair (k, j) is INVALID
 *   if a Q is not finite or |Q| >= 2^40, and then contributes to no word; otherwise v = Q >> 10 (floor) is the voxel whose
 *   mlm_export_window entry is read, as in mlm_query_nearest.  A NaN or an infinity anywhere in pts_s or T_ws is no error.
 *   Classes (read only with MLM_SCORE_CLASSES): occ and infl are what mlm_export_window's channels return at v — absent blocks,
 *   released frontier-mode blocks (element 0 answers, inflated class UNKNOWN) and voxels beyond the key range (UNKNOWN) included.
 *   Field: lo, dims and sqdist are all NULL or all given.  The window follows mlm_export_window's rules and errors; sqdist holds one
 *   int32 per voxel, laid out [dims[2]][dims[1]][dims[0]]: what mlm_export_esdf wrote for that box, unsigned or signed.  sq_cap lies
 *   in 1 .. 2^20.  The answer is defined for any content of sqdist: the cost of a valid pair is min(max(sqdist[v], 0), sq_cap) if v
 *   lies in the box, sq_cap otherwise.
 *   Row k of table (int64 [n_poses][MLM_SCORE_ROW]; all eight words are always written):
 *     [0] valid pairs
 *     [1] pairs with occ == OCCUPIED                       (CLASSES, else 0)
 *     [2] pairs with occ == FREE                           (CLASSES, else 0)
 *     [3] pairs with occ == UNKNOWN                        (CLASSES, else 0)
 *     [4] pairs with infl == OCCUPIED                      (CLASSES, else 0)
 *     [5] valid pairs whose voxel lies in the box          (field, else 0)
 *     [6] sum of the costs over the valid pairs            (field, else 0)
 *     [7] valid pairs in the box with sqdist[v] <= 0       (field, else 0)
 *   [1] + [2] + [3] == [0].  Every word is a count or a sum of integers, below 2^43, with one value whatever the schedule.  For a
 *   matcher: [6] small and [1] large mean the frame lies on the map's surfaces; [2] counts returns from inside known free space
 *   (something new, or a wrong pose); [3] counts returns the map cannot judge.
 * pts_s, T_ws, sqdist and table may each be host or device memory.  The call runs on the stream of mlm_set_stream and returns when
 * table is written.  With MLM_SCORE_CLASSES it observes the map as queries do (async mode: waits for everything submitted); without,
 * it reads no map state and does not wait, as mlm_query_paths.  When every array is host memory, n_poses * n_pts <= 2^16 and n_poses
 * is at most what mlm_query_nearest allows points (64; 8 while the host mirror needs a refresh), the batch is answered on the host
 * without a launch (same answers): from the host mirror with CLASSES, by the same host code with no mirror without.  Everything
 * else, and every batch after mlm_set_host_mirror_limit(h, 0), runs as a kernel.  MLM_ERR_INVALID: n_pts or n_poses outside
 * 0 .. 2^22, a NULL input with a count > 0, table NULL, an unknown flag bit, neither CLASSES nor a field, lo / dims / sqdist only
 * partly given, a window error, sq_cap outside 1 .. 2^20 with a field; n_poses == 0 is MLM_OK, n_pts == 0 writes zero rows.
 * MLM_ERR_CAPACITY: no device memory for the staging of host pts_s (24 bytes x n_pts), T_ws (96 bytes) and table (64 bytes per pose,
 * at most 2^18 poses at a time; each part rounded up to 256 bytes, in the buffer mlm_query_rays stages in), or for the kept device
 * copy of a host sqdist (4 bytes per voxel, a buffer of its own); both are kept by the handle and counted in
 * mlm_frame_stats.device_bytes.  The handle stays usable after either error. */
#define MLM_SCORE_CLASSES 1
#define MLM_SCORE_ROW 8
int mlm_score_poses(mlm_handle *h, const double *pts_s, int n_pts, const double *T_ws, int n_poses, int flags,
                    const int32_t lo[3], const int32_t dims[3], const int32_t *sqdist, int sq_cap, int64_t *table);
/* Exact batched segment casts through a distance field: "is the piece from a to b free for a vehicle of radius r, how close does it
 * come to an obstacle, where, and what does that cost?" — the edge check and the edge weight of a sampling planner, from a field the
 * caller already holds.  (No reference counterpart: the reference has no segment query and no distance field; the path is
 * mlm_query_rays', the field is mlm_export_esdf's sqdist, the rule is defined here, in integers, with exactly one answer.)  Segment i
 * runs from p0[3i .. 3i+2] to p1[3i .. 3i+2].  The lattice, the validity rule, the path u_0 .. u_N, the tie rule of the walk and t are
 * mlm_query_rays'.
 *   Field: lo, dims and sqdist are required.  The window follows mlm_export_window's rules and errors; sqdist holds one int32 per
 *   voxel, laid out [dims[2]][dims[1]][dims[0]]: what mlm_export_esdf wrote for that box, unsigned or signed, but the answer is defined
 *   for any content: f(v) = min(max(sqdist[v], 0), sq_cap) for v in the box.  sq_cap lies in 1 .. 2^20, sq_stop in -1 .. 2^20 (-1:
 *   nothing stops the walk).
 *   Stop: the walk stops at K, the smallest path index for which u_K lies outside the box and MLM_CLEAR_OUTSIDE_PASS is not set (status
 *   MLM_CLEAR_LEFT), or f(u_K) <= sq_stop (status 1); without one K = N + 1 and status is 0.  With MLM_CLEAR_OUTSIDE_PASS a voxel
 *   outside the box has f = sq_cap (mlm_score_poses' rule) and only the second test is made: such a voxel stops the walk iff
 *   sq_cap <= sq_stop.  Passed = u_0 .. u_{K-1}; seen = passed, plus u_K at status 1.
 *   Per ray:                status 1 / 2                         status 0      invalid
 *     status     int8       1 (the field) / MLM_CLEAR_LEFT       0             -1
 *     voxel3     int32 x 3  u_K                                  e             0,0,0
 *     t          double     (double)m / (double)|D| of the step  1.0           0.0
 *                           that entered u_K; 0.0 for K = 0
 *     n_steps    int32      K                                    N + 1         0
 *     min_sq     int32      the minimum of f over seen; MLM_CLEAR_NONE when seen is empty        MLM_CLEAR_NONE
 *     min3       int32 x 3  the seen voxel of smallest path index attaining min_sq; 0,0,0 with MLM_CLEAR_NONE
 *     cost       int64      the sum over passed of sq_cap - f, at most (3 * 2^15 + 1) * 2^20      0
 *     n_near     int32      the passed voxels with f < sq_cap                                     0
 *   At status 1 min_sq == f(u_K) <= sq_stop and min3 == voxel3.  With a field of mlm_export_esdf at max_dist r + 1, sq_stop = r^2 and
 *   every path inside the box, status, voxel3, t and n_steps are mlm_query_sweeps' bytes at radius r with the same class bits, and
 *   min_sq at a stop is its hit_sq: an edge checked here agrees voxel for voxel with mlm_export_reach / mlm_export_route about "free
 *   for radius r".
 *   Groups (group_begin and table both given or both NULL): group_begin is int32 [n_groups + 1], first entry >= 0, non-decreasing,
 *   last entry <= n (validated on the host, as mlm_query_views' view_begin); group g is the segments group_begin[g] ..
 *   group_begin[g + 1] - 1 in index order (a trajectory's pieces; the end points need not join; rays in no group are allowed).  j* is
 *   the first segment of the group with status != 0 (an invalid one counts), C the segments from the group's first to j* inclusive, or
 *   all of them without one.  Row g of table (int64 [n_groups][MLM_CLEAR_ROW]): [0] segments in the group, [1] j* - begin or -1,
 *   [2] status of j* or 0, [3] the minimum of min_sq over C, ignoring MLM_CLEAR_NONE; -1 if there is none, [4] the index within the group
 *   of the first segment attaining [3] or -1, [5] the sum of cost over C, [6] of n_steps, [7] of n_near.  The row does not depend on
 *   which per-ray outputs were requested.
 * Every pointer but lo and dims may be host or device memory, each on its own.  Any output may be NULL (table counts as one), at least
 * one must not be.  The call reads no map state and waits for no frame, as mlm_query_paths; it runs on the stream of mlm_set_stream and
 * returns when the outputs are written.  When every array is host memory, n <= 64, the valid rays' sum of N + 1 is at most 2^18 and the
 * host mirror is not switched off (mlm_set_host_mirror_limit(h, 0)), the batch is answered on the host by the same rule, with no launch
 * and no copy (counted in mlm_frame_stats.n_host_queries); everything else runs as a kernel: a host sqdist crosses the link once into
 * the buffer mlm_score_poses keeps for its field, host rays and outputs are staged in chunks of 2^18 rays (at most 101 bytes per ray,
 * each part rounded up to 256 bytes, in the buffer mlm_query_rays stages in), and with groups 21 bytes per ray of the whole batch plus a
 * host group_begin and table live in a kept scratch; all of it is counted in mlm_frame_stats.device_bytes.  MLM_ERR_INVALID: n < 0, a
 * NULL input with n > 0, a NULL lo, dims or sqdist, a window error, sq_stop outside -1 .. 2^20, sq_cap outside 1 .. 2^20, an unknown
 * flag bit, no output, group_begin and table not both given or both NULL, n_groups < 0, a bad group_begin; n == 0 with n_groups == 0
 * is MLM_OK (n == 0 with groups writes their rows).  MLM_ERR_CAPACITY: no device memory for staging, scratch or the field copy.  The
 * handle stays usable after either error. */
#define MLM_CLEAR_OUTSIDE_PASS 1 /* path voxels outside the box have f = sq_cap and never end the walk by leaving */
#define MLM_CLEAR_NONE (-1)      /* min_sq of a ray that saw no voxel */
#define MLM_CLEAR_LEFT 2         /* status: the walk reached a path voxel outside the box */
#define MLM_CLEAR_ROW 8          /* int64 per group row */
int mlm_query_clearance(mlm_handle *h, const double *p0, const double *p1, int n,
                        const int32_t lo[3], const int32_t dims[3], const int32_t *sqdist, int sq_stop, int sq_cap, int flags,
                        int8_t *status, int32_t *voxel3, double *t, int32_t *n_steps,
                        int32_t *min_sq, int32_t *min3, int64_t *cost, int32_t *n_near,
                        const int32_t *group_begin, int n_groups, int64_t *table);
/* Cost-to-go field through the free space of a box of voxels (no reference counterpart: the reference has no such field; the
 * classes behind it are those of its point queries, the field is defined here, in integers).  Voxel indices, window, layout
 * ([dims[2]][dims[1]][dims[0]], x fastest) and centres are those of mlm_export_window.
 *   Obstacles: O(v) is the union of what `flags` selects — MLM_REACH_OCC getOccupancy(centre) == OCCUPIED, MLM_REACH_INFL
 *   getInflateOccupancy(centre) == OCCUPIED, MLM_REACH_UNKNOWN getOccupancy(centre) == UNKNOWN — i.e. mlm_export_esdf's predicate
 *   on what mlm_export_window's occ / infl channels return at v (released frontier-mode blocks, absent blocks and voxels beyond
 *   the key range included).  flags == 0: no obstacles (as in mlm_query_rays).
 *   Clearance r (0..63 voxels, the robot's radius): a voxel v is BLOCKED if some voxel o of the whole map (not only the box) has
 *   O(o) and |v - o|^2 <= r^2 (integer squared index distance; r = 0: blocked iff O(v)): D_out(v) <= r^2 of mlm_export_esdf at
 *   max_dist = r + 1, computed by the same passes.
 *   Traversable: T(v) iff v lies in the box and is not blocked.  The domain is the box: a path never leaves it (obstacles are
 *   looked up beyond it, paths are not; a caller who wants more context asks for a larger box).
 *   Seeds: n_seeds >= 1 absolute voxel index triples (host or device memory).  A seed outside the box or not traversable
 *   contributes nothing and is no error (the voxel that holds the vehicle is UNKNOWN in a fresh map: with MLM_REACH_UNKNOWN seed the
 *   nearest traversable voxel instead); the others are the effective seeds.  Duplicates are allowed.
 *   steps  int32  the smallest number of moves of a 6-connected path seed = v0, v1, ..., vk = v whose voxels are all traversable,
 *                 over all effective seeds; 0 at an effective seed; MLM_REACH_NONE if v is not traversable, if there is no such
 *                 path, or if that number exceeds max_steps (1 <= max_steps <= 2^31 - 1; values <= max_steps are what they are
 *                 without the truncation)
 *   parent uint8  at a reached voxel that is no seed the lowest code c whose neighbour v + e_c lies in the box and has
 *                 steps == steps(v) - 1, codes 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z; MLM_REACH_SEED at effective seeds; 255
 *                 where steps is MLM_REACH_NONE.  Following parent from a reached voxel walks one shortest path to a seed.
 *   summary int64 x 4 (host memory): [0] traversable voxels of the box, [1] reached voxels, [2] the largest steps written (-1:
 *                 none), [3] relaxation sweeps the call needed (informative: depends on the tile geometry).
 * steps and parent may be host or device memory; any of the three outputs may be NULL, at least one must not be.  The field is
 * the least fixpoint of steps(v) = min(steps(v), 1 + min over traversable neighbours) from the seeds, so it has exactly one value
 * whatever the schedule.  The call observes the map as queries do (async mode: waits for everything submitted), runs on the
 * stream of mlm_set_stream and returns when the outputs are written.  MLM_ERR_INVALID: mlm_export_window's window errors,
 * n_seeds < 1 or seeds3 == NULL, an unknown flag bit, clearance outside [0, 63], max_steps < 1, no output.  MLM_ERR_CAPACITY:
 * no device memory for the scratch: this is a global problem that cannot be cut into independent tiles, so the whole box's
 * field (4 bytes per voxel), one mask byte per voxel and two dirty bytes per tile are resident at once (plus the ESDF scratch
 * with clearance > 0 and a staging copy of host outputs), kept by the handle and counted in mlm_frame_stats.device_bytes.  The
 * handle stays usable after either error. */
#define MLM_REACH_OCC 1 /* same bits and same meaning as MLM_ESDF_OCC / _INFL / _UNKNOWN */
#define MLM_REACH_INFL 2
#define MLM_REACH_UNKNOWN 4
#define MLM_REACH_NONE (-1) /* steps of a voxel that is not reached */
#define MLM_REACH_SEED 6    /* parent code of a seed */
int mlm_export_reach(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], const int32_t *seeds3, int n_seeds,
                     int flags, int clearance, int max_steps, int32_t *steps, uint8_t *parent, int64_t summary[4]);
/* Clearance-weighted cost field through the free space of a box of voxels, with face, edge and corner moves (no reference
 * counterpart: the reference has no such field; it is defined here, in integers).  What a planner with diagonal moves and a soft
 * clearance cost searches on: mlm_export_reach's paths are Manhattan staircases that hug obstacles at exactly `clearance` voxels.
 * Window, layout, voxel indices, the obstacle predicate O(v) of `flags`, the clearance r (v is BLOCKED iff D_out(v) <= r^2, looked
 * up in the whole map), traversable voxels, the domain (the box: a path never leaves it) and the seeds (host or device memory; one
 * outside the box or on a blocked voxel contributes nothing; duplicates allowed) are those of mlm_export_reach.
 *   Moves: connectivity 6, 18 or 26 — the offsets of {-1, 0, 1}^3 with one, at most two, at most three non-zero entries, as in
 *   mlm_export_clusters.  A move by offset o from u to v = u + o costs move_cost[nnz(o) - 1] (host memory, each entry in 1..65535;
 *   entries of move kinds the connectivity excludes are ignored).  It is permitted iff u and v are traversable voxels of the box
 *   and so is u + o' for every o' obtained from o by zeroing a non-empty proper subset of its non-zero entries: an edge move needs
 *   its two face-adjacent intermediates, a corner move its six intermediates (no corner cutting; that is the whole rule, and it is
 *   symmetric in u and v).  Voxels outside the box count as blocked.
 *   Soft clearance: penalty (host memory) has n_penalty >= 0 entries, each in 0..65535, clearance + n_penalty <= 63; NULL iff
 *   n_penalty == 0.  The ring k(v) of a traversable v is the smallest k >= 0 with D_out(v) <= (r + 1 + k)^2; pen(v) = penalty[k(v)]
 *   if k(v) < n_penalty, else 0.  D_out is mlm_export_esdf's, computed by the same passes at max_dist = r + n_penalty + 1, so every
 *   threshold lies strictly below the truncation; with n_penalty == 0 the blocked mask is obtained exactly as mlm_export_reach
 *   obtains it.
 *   cost   int32  the cost of a path v0 ... vk of permitted moves from an effective seed v0 is the sum over i = 1..k of
 *                 move_cost(move i) + pen(v_i) (a seed costs 0 and pays no penalty for its own voxel); cost(v) is the minimum over
 *                 all such paths from all effective seeds; MLM_ROUTE_NONE if v is not traversable, if there is no path, or if
 *                 the minimum exceeds max_cost (1 <= max_cost <= 2^31 - 1; values <= max_cost are what they are without the
 *                 truncation)
 *   parent uint8  at a reached voxel that is no seed the lowest code c such that the move from u = v + o_c to v is permitted and
 *                 cost(u) + move_cost + pen(v) == cost(v); MLM_ROUTE_SEED at effective seeds; 255 where cost is MLM_ROUTE_NONE.
 *                 Codes 0..5 are mlm_export_reach's (-x, +x, -y, +y, -z, +z); 6..17 the twelve offsets with two non-zero entries
 *                 in ascending lexicographic order of (dz, dy, dx): 6 is (dx, dy, dz) = (0, -1, -1), 10 is (-1, -1, 0), 17 is
 *                 (0, 1, 1); 18..25 the eight corners in the same order: 18 is (-1, -1, -1), 25 is (1, 1, 1).  Face moves win ties.
 *                 Following parent from a reached voxel walks one optimal path to a seed.
 *   summary int64 x 4 (host memory): [0] traversable voxels of the box, [1] reached voxels, [2] the largest cost written (-1:
 *                 none), [3] relaxation sweeps the call needed (informative: depends on the tile geometry).
 * cost and parent may be host or device memory; any of the three outputs may be NULL, at least one must not be.  The field is the
 * least fixpoint of cost(v) = min(cost(v), cost(u) + move_cost + pen(v)) over permitted moves, so it has exactly one value
 * whatever the schedule.  With connectivity 6, move_cost[0] == 1, n_penalty == 0 and max_cost == max_steps, cost and parent equal
 * mlm_export_reach's steps and parent, with the seed code MLM_ROUTE_SEED (26) in place of MLM_REACH_SEED (6).  Streams, async
 * mode and mlm_frame_stats.device_bytes as for mlm_export_reach, whose scratch the call shares.  MLM_ERR_INVALID:
 * mlm_export_reach's window, seed and flag errors, clearance outside [0, 63], connectivity other than 6 / 18 / 26, move_cost NULL
 * or an entry out of range, n_penalty < 0, clearance + n_penalty > 63, penalty NULL with n_penalty > 0 or an entry out of range,
 * max_cost < 1, no output.  MLM_ERR_CAPACITY: as for mlm_export_reach — the whole box is resident, 4 bytes of cost and one class
 * byte per voxel, two dirty bytes per tile (plus the ESDF scratch with clearance + n_penalty > 0 and a staging copy of host
 * outputs).  The handle stays usable after either error. */
#define MLM_ROUTE_OCC 1 /* same bits and meaning as MLM_REACH_* */
#define MLM_ROUTE_INFL 2
#define MLM_ROUTE_UNKNOWN 4
#define MLM_ROUTE_NONE (-1) /* cost of a voxel that is not reached */
#define MLM_ROUTE_SEED 26   /* parent code of an effective seed */
int mlm_export_route(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], const int32_t *seeds3, int n_seeds,
                     int flags, int clearance, int connectivity, const int32_t move_cost[3],
                     const int32_t *penalty, int n_penalty, int max_cost,
                     int32_t *cost, uint8_t *parent, int64_t summary[4]);
/* Paths through a parent field, traced and shortened to way points (no reference counterpart: the reference has neither a cost field
 * nor a path query; the rule is defined here, in integers, with exactly one answer).  The call reads the field it is given and no map
 * state.  Window (lo, dims), layout ([dims[2]][dims[1]][dims[0]], x fastest) and errors are those of mlm_export_window.
 *   Field: `parent` holds one byte per voxel of the box: what mlm_export_reach (kind MLM_PATH_REACH, M = 6) or mlm_export_route (kind
 *   MLM_PATH_ROUTE, M = 26) wrote for it.  Bytes 0 .. M - 1 are moves with the offsets of mlm_export_route's codes (the first six are
 *   mlm_export_reach's), M is a seed.  open(v) iff v lies in the box and parent[v] <= M.  The answer is defined, and the call ends, for
 *   any content of `parent`: nothing relies on the field being genuine.
 *   Trace: goal i is the absolute voxel goals3[3i .. 3i+2].  Outside the box or not open: status 0, table row all zero.  Else u_0 =
 *   goal, k = 0, and in this order: c = parent[u_k]; if c == M: status 1, K = k, stop; if k == max_moves: status -1 (too long), K = k,
 *   stop; u' = u_k + offset(c); if u' is outside the box or not open: status -2 (broken field), K = k, stop; else u_{k+1} = u', k += 1.
 *   Visibility: vis(a, b), for open voxels a, b with |b_x - a_x| <= lookahead on every axis, in integers: n_x = |b_x - a_x|, s_x =
 *   sign(b_x - a_x); a walk starts at c = a with counters k_x = 0; while c != b: of the axes with k_x < n_x take the smallest crossing
 *   parameter (2 k_x + 1) / (2 n_x) (compared by cross-multiplication) and the set T of all axes that attain it (1, 2 or 3 axes); for
 *   every non-empty subset S of T the voxel c + sum over S of s_x e_x must be open, else vis is false; then c += sum over T of
 *   s_x e_x and k_x += 1 for x in T.  This is mlm_query_rays' path between the two voxel centres plus every voxel the segment grazes at
 *   an exact edge or corner tie; for a unit offset it is mlm_export_route's permitted-move rule, so a shortened path cuts no corner
 *   the field's own moves may not cut; vis(a, b) == vis(b, a).  An open voxel is a reached traversable voxel, so every voxel under a
 *   shortened leg keeps the field's hard clearance; the soft penalty is not re-optimised: the shortening is geometric.
 *   Shortening (status 1; L = lookahead, 1 .. 4096): i_0 = 0, i_{t+1} = max{ j : i_t < j <= min(K, i_t + L), j == i_t + 1 or
 *   vis(u_{i_t}, u_j) }, until i_t == K.  The maximum is over all j of the window, not over the first run of visible ones.  The way
 *   points are u_{i_0} .. u_{i_{W-1}}, goal first, seed last; W = 1 for a goal that is a seed; L = 1 returns the raw path, W = K + 1.
 *   Per goal:
 *     status  int8               1, 0, -1 or -2 as above
 *     way3    int32 [cap][3]     status 1: the first min(W, cap) way points as absolute voxel indices, rows beyond left as they were;
 *                                nothing is written at another status.  cap >= 0; cap == 0 iff way3 == NULL.
 *     length  double             status 1: the way-point polyline in metres: acc = 0.0, then for t = 0 .. W - 2 in order
 *                                acc = acc + ((double)(float)subbox_d_xyz * sqrt((double)sq_t)), sq_t the integer squared voxel length
 *                                of leg t; every operation one IEEE double operation, nothing fused, sqrt correctly rounded; all legs
 *                                count, whatever cap.  -1.0 at another status.
 *     table   int64 [MLM_PATH_ROW]  [0] K (at status -1 and -2 too: the moves taken); at status 1 also [1] W, [2] [3] [4] the face, edge
 *                                and corner moves of the raw path, [5] the longest leg in moves (max of i_{t+1} - i_t; 0 for W = 1),
 *                                [6] the sum over t of min(K, i_t + L) - i_{t+1}: the candidates beyond the chosen one, [7] 0;
 *                                otherwise [1 .. 7] are 0.
 * parent, goals3 and each output on its own may be host or device memory; any output may be NULL, at least one must not be.  The call
 * takes the handle's lock, runs on the stream of mlm_set_stream and returns when the outputs are written; it does not read the map,
 * so it does not wait for submitted frames.  With parent in host memory the whole call runs on the host (same rule, same answers; no
 * launch, no copy of the field; goals and outputs in device memory are copied across); with parent in device memory it runs as a
 * kernel, host goals and outputs staged in mlm_query_rays' buffer.  MLM_ERR_INVALID: the window errors, parent NULL, kind not 0 or 1,
 * n < 0 or goals3 NULL with n > 0, lookahead outside [1, 4096], max_moves outside [1, 2^20], cap < 0 or at odds with way3, no output;
 * n == 0 is MLM_OK.  MLM_ERR_CAPACITY: no device memory for the path scratch (12 bytes x (max_moves + 1) per goal, taken for chunks of
 * goals of at most 256 MiB, kept by the handle and counted in mlm_frame_stats.device_bytes) or for the staging (85 + 12 cap bytes per
 * goal, chunks of at most 64 MiB).  The handle stays usable after either error. */
#define MLM_PATH_REACH 0 /* parent field of mlm_export_reach: move codes 0..5,  seed code 6  */
#define MLM_PATH_ROUTE 1 /* parent field of mlm_export_route: move codes 0..25, seed code 26 */
#define MLM_PATH_ROW 8
int mlm_query_paths(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], const uint8_t *parent, int kind,
                    const int32_t *goals3, int n, int lookahead, int max_moves, int cap,
                    int8_t *status, int32_t *way3, double *length, int64_t *table);
/* Connected components of a voxel set of a box, with per-component statistics (no reference counterpart: the reference has no
 * clustering, its visualiser publishes the frontier cloud raw; the classes behind the set are those of its point queries, set,
 * components and numbering are defined here, in integers).  Voxel indices, window, layout ([dims[2]][dims[1]][dims[0]], x
 * fastest) and centres are those of mlm_export_window.
 *   The set S: `flags` is either MLM_CLUSTER_FRONTIER alone or a non-empty union of MLM_CLUSTER_OCC / _INFL / _UNKNOWN.  The class
 *   bits: S(v) iff v lies in the box and mlm_export_esdf's obstacle predicate O(v) holds.  FRONTIER: S(v) iff v lies in the box,
 *   occ(v) == FREE and occ(u) == UNKNOWN for at least one of the six face neighbours u of v, occ being what mlm_export_window's occ
 *   channel returns; neighbours are looked up in the whole map, also outside the box (released frontier-mode blocks and absent
 *   blocks included); a neighbour whose index leaves int32 is UNKNOWN (no block can hold it).  Unlike mlm_export_frontier this
 *   does not need frontier mode and works on any handle (a map loaded with mlm_import_blocks, a merged one).
 *   Components: connectivity 6, 18 or 26 — moves by the offsets of {-1, 0, 1}^3 with one, at most two, at most three non-zero
 *   entries.  Two voxels of S are in one component iff a chain of such moves joins them through voxels of S inside the box (the
 *   domain is the box, as in mlm_export_reach).  The root of a component is its voxel with the smallest linear box index
 *   (z * dims[1] + y) * dims[0] + x.
 *   Numbering: components of at least min_size (>= 1) voxels are kept and numbered 0 .. K-1 in ascending order of their roots, so
 *   every output is a function of the map and the arguments alone.
 *   labels int32 per voxel: the number of its kept component; MLM_CLUSTER_SMALL in a dropped one; MLM_CLUSTER_NONE off S.
 *   table  int64 [cap][MLM_CLUSTER_ROW], row k for kept component k < cap (K > cap is no error: the first cap rows are written,
 *          labels is complete, summary[2] tells; rows from K on are left as they were): [0] voxels; [1..3] root, absolute x, y,
 *          z; [4..6] / [7..9] smallest / largest absolute index per axis; [10..12] sum over the component of x - lo[0],
 *          y - lo[1], z - lo[2] (centroid = lo + sum / voxels; < 2^62 by the window limits); [13] bit c set iff the component
 *          has a voxel on face c of the box (0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z) — a cluster the box has cut; [14], [15] 0.
 *   summary int64 x 6 (host memory): [0] voxels of S in the box, [1] components of any size, [2] K, [3] voxels in kept components,
 *          [4] the largest component (0: none), [5] informative, depends on the tile geometry: the most passes a tile with a
 *          voxel of S needed to settle its own piece (>= 1 when S is not empty).
 * labels and table may each be host or device memory; any of the three outputs may be NULL, at least one must not be; cap >= 0,
 * cap == 0 iff table == NULL.  "Every voxel is labelled with the smallest index of its component" is a least fixpoint of values
 * that only decrease, so there is exactly one result whatever the schedule.  The call observes the map as queries do (async
 * mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns when the outputs are written.
 * MLM_ERR_INVALID: mlm_export_window's window errors, flags that are neither of the two forms, connectivity other than 6 / 18 /
 * 26, min_size < 1, cap < 0 or at odds with table, no output.  MLM_ERR_CAPACITY: no device memory for the scratch: a global
 * problem like mlm_export_reach, so the whole box is resident at once — the label word (4 bytes per voxel), one mask byte per
 * voxel, for the numbering a second word per voxel (the size of a component at its root, then its number) and one count per
 * 2048 voxels (kept roots, scanned), for FRONTIER the occ class of the box grown by one voxel per side (1 byte each), and for
 * host destinations min(cap, voxels) rows and a staging copy of labels; kept by the handle and counted in
 * mlm_frame_stats.device_bytes.  The handle stays usable after either error. */
#define MLM_CLUSTER_OCC 1       /* same bits and same meaning as MLM_ESDF_OCC / _INFL / _UNKNOWN */
#define MLM_CLUSTER_INFL 2
#define MLM_CLUSTER_UNKNOWN 4
#define MLM_CLUSTER_FRONTIER 16 /* getOccupancy(centre) == FREE and a 6-neighbour's getOccupancy(centre) == UNKNOWN */
#define MLM_CLUSTER_NONE (-1)   /* label of a voxel outside the set */
#define MLM_CLUSTER_SMALL (-2)  /* label of a voxel of the set whose component has fewer than min_size voxels */
#define MLM_CLUSTER_ROW 16      /* int64 per table row */
int mlm_export_clusters(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, int connectivity, int min_size,
                        int32_t *labels, int64_t *table, int cap, int64_t summary[6]);
/* Exact indexed surface mesh of the obstacle set of a box: the voxel faces between an obstacle and an open voxel, as quads over
 * shared vertices (no reference counterpart: the reference has no mesh, its visualiser publishes point clouds; the classes behind
 * the set are those of its point queries, faces, vertices and numbering are defined here, in integers).  Voxel indices, window,
 * layout and centres are those of mlm_export_window; the classes are what its occ / infl channels return (released frontier-mode
 * blocks and absent blocks included); a voxel whose index leaves int32 or the key range is UNKNOWN, as in mlm_export_clusters.
 *   O(v): mlm_export_esdf's obstacle predicate for MLM_MESH_OCC / _INFL / _UNKNOWN (at least one of them is required).
 *   open(u): !O(u); with MLM_MESH_SEEN !O(u) and occ(u) == FREE — a wall's never-observed back side has no faces.
 *   Voxels outside the box are looked up in the whole map, so the meshes of adjacent boxes fit together without a seam or a doubled
 *   face.  With MLM_MESH_CLOSED they are open and no obstacles whatever the other flags say: the mesh is then the closed boundary
 *   of the box's obstacle set.
 *   Faces: a face is a pair (v, a) with v in the box, O(v) and open(v + e_a); a = 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z (the face
 *   numbering of mlm_export_clusters' row word 13).  Faces are numbered 0 .. F-1 in ascending order of linear(v) * 6 + a, linear(v)
 *   = (z * dims[1] + y) * dims[0] + x in the box.
 *   Vertices: lattice point k, lo[i] <= k[i] <= lo[i] + dims[i] (dims + 1 points per axis), is the lower corner of voxel k.  It is
 *   a vertex iff it is a corner of at least one face; vertices are numbered 0 .. V-1 in ascending lattice linear index, x fastest.
 *   quads    int32 [cap_faces][4]: the vertex numbers of the face's corners, counter-clockwise seen from the open side.  With
 *            u = a >> 1, p = (u + 1) % 3, q = (u + 2) % 3 and b = v + (a & 1) e_u: b, b + e_p, b + e_p + e_q, b + e_q for odd a and
 *            b, b + e_q, b + e_p + e_q, b + e_p for even a, so that (c1 - c0) x (c3 - c0) is the outward unit normal.  Triangles:
 *            (0, 1, 2) and (0, 2, 3).
 *   face4    int32 [cap_faces][4]: absolute x, y, z of v, then a — the surface element an inspection planner samples views from.
 *   vert3    int32 [cap_verts][3]: the absolute lattice coordinates.
 *   vert_xyz float [cap_verts][3]: per axis, with g = floor(k / subbox_n) and c = k - g * subbox_n,
 *            (float)((double)g * (subbox_d_xyz * subbox_n) + (double)c * subbox_d_xyz), evaluated in IEEE double in that order,
 *            uncontracted, rounded once: the voxel centre's formula without its + d / 2.
 *   vert_n3  int8 [cap_verts][3]: the sum of the outward unit normals of the faces the vertex is a corner of, each component in
 *            -4 .. 4 (normalise it for smooth shading; (0, 0, 0) at a pinch point).
 *   summary  int64 x MLM_MESH_ROW (host memory): [0] F, [1] V, [2] obstacle voxels in the box, [3] those with at least one face,
 *            [4..9] faces per direction 0..5, [10] faces whose open neighbour lies outside the box, [11] 0.
 * F > cap_faces or V > cap_verts is no error: the first cap rows are written, rows beyond stay as they were, summary tells, and quads
 * always carry the true vertex numbers; a call with only summary sizes the next one.  Every array may be host or device memory; any
 * pointer may be NULL, at least one of the six must not be; a cap is 0 iff all of its arrays are NULL.  Ranks in a fixed order, no
 * order of arrival anywhere: there is exactly one result whatever the schedule.  The call observes the map as queries do (async
 * mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns when the outputs are written.
 * MLM_ERR_INVALID: mlm_export_window's window errors, more than 2^31 - 1 lattice points (every vertex number fits an int32), none
 * of the three class bits or an unknown bit, a negative cap or a cap at odds with its arrays, no output.  MLM_ERR_CAPACITY: no
 * device memory for the scratch: the whole box is resident at once, as for mlm_export_clusters — per voxel one face-mask byte and
 * one state byte (the latter for the box grown by one voxel per side), per lattice point 3/16 byte (a vertex bit and a 32-bit
 * base per 64 of them), 8 bytes per 2048 voxels and per 2048 lattice points, and for host destinations a staging copy of at most
 * 2^20 rows per array; kept by the handle and counted in mlm_frame_stats.device_bytes.  The handle stays usable after either
 * error. */
#define MLM_MESH_OCC 1      /* same bits and same meaning as MLM_ESDF_OCC / _INFL / _UNKNOWN */
#define MLM_MESH_INFL 2
#define MLM_MESH_UNKNOWN 4
#define MLM_MESH_SEEN 16    /* only faces towards a voxel with getOccupancy == FREE */
#define MLM_MESH_CLOSED 32  /* every voxel outside the box counts as open and as no obstacle */
#define MLM_MESH_ROW 12     /* int64 in summary */
int mlm_export_mesh(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int flags, int32_t *quads, int32_t *face4,
                    int64_t cap_faces, int32_t *vert3, float *vert_xyz, int8_t *vert_n3, int64_t cap_verts,
                    int64_t summary[MLM_MESH_ROW]);
/* Exact pruned occupancy octree of a box: occupied, free and absent cubes sized by how uniform the space is, the structure of
 * OctoMap's binary tree (no reference counterpart: the reference publishes flat point markers; the classes behind the labels are
 * those of its point queries, tree and numbering are defined here, in integers).  Voxel indices, window and layout are those of
 * mlm_export_window; the classes are what its occ / infl channels return.
 *   Classes: a voxel is OCC if occ == OCCUPIED, with MLM_OCT_INFL also if infl == OCCUPIED; FREE if occ == FREE and it is not OCC;
 *   NONE otherwise — absent blocks, released frontier-mode blocks that say UNKNOWN and indices outside the key range included, as in
 *   mlm_export_mesh.  Voxels outside the box are NONE and are not looked up.  With MLM_OCT_OCC_ONLY FREE voxels are NONE too (the small
 *   tree a visualiser wants).
 *   Tree: depth D is 1..31 and every index of the box lies in [-2^(D-1), 2^(D-1)).  The key of an index is k = index + 2^(D-1) per
 *   axis; the level-l cell of a key is k >> l, on the absolute lattice, so the trees of adjacent boxes share their cell boundaries
 *   (D = 16 is OctoMap's key space).  The root is the one level-D cell.  Child i of a cell takes bit 0 of i from x, bit 1 from y
 *   and bit 2 from z of the next key bit.  The label of a level-0 cell is its voxel's class; a cell of level l > 0 is NONE if all
 *   eight children are NONE, an OCC leaf if all eight are OCC leaves, a FREE leaf if all eight are FREE leaves, INNER otherwise: the
 *   canonical pruned tree.
 *   Numbering: depth-first pre-order, children in order 0..7; the inner nodes are numbered 0 .. N-1 and the leaves 0 .. M-1 in that
 *   order (for the leaves the Morton order of their lower corners).
 *   words      uint16 [cap_inner]: the sum over the children i of label << 2i, NONE 0, FREE 1, OCC 2, INNER 3; stored little-endian,
 *              the stream is meant to be the payload of OctoMap's binary tree file.
 *   inner4     int32 [cap_inner][4]: the cell's lower corner as voxel index x, y, z, then its level.
 *   skip       int32 [cap_inner]: n + the inner nodes in n's subtree (n included): the next inner node outside the subtree — a
 *              stackless traversal.
 *   leaf4      int32 [cap_leaves][4]: lower corner x, y, z, then level.
 *   leaf_class int8 [cap_leaves]: 0 OCCUPIED or 1 FREE.
 *   summary    int64 x MLM_OCT_ROW (host memory): [0] N, [1] M, [2] OCC leaves, [3] FREE leaves, [4] OCC voxels, [5] FREE voxels, [6] the
 *              root's label, [7] 0, [8 + l] leaves at level l, l = 0..31.
 * N > cap_inner or M > cap_leaves is no error: the first cap rows are written, rows beyond stay as they were, summary tells; a call
 * with only summary sizes the next one.  Every array may be host or device memory; any pointer may be NULL, at least one of the six
 * must not be; a cap is 0 iff all of its arrays are NULL.  The labels are a function of the classes, the numbers an exclusive prefix
 * over eight children, top-down: there is exactly one result whatever the schedule.  The call observes the map as queries do (async
 * mode: waits for everything submitted), runs on the stream of mlm_set_stream and returns when the outputs are written.
 * MLM_ERR_INVALID: mlm_export_window's window errors, more than 2^31 - 1 voxels, depth outside 1..31 or a box that leaves the key cube,
 * an unknown flag bit, a negative cap or a cap at odds with its arrays, no output.  MLM_ERR_CAPACITY: no device memory for the
 * scratch: with T = min(D, 4) and C the cells of levels T..D that meet the box (per level the product over the axes of
 * ((khi - 1) >> l) - (klo >> l) + 1 for the box's keys [klo, khi)), up(C) + 4 up(4 C) + 1024 bytes, up() rounding up to a multiple
 * of 256 — 17 bytes per 16^3 brick and a little for the levels above; nothing is stored per voxel, the levels below a brick's top
 * are recomputed where the rows are written —, and for host destinations a staging copy of at most 2^20 rows per array; kept by the
 * handle and counted in mlm_frame_stats.device_bytes.  The handle stays usable after either error. */
#define MLM_OCT_INFL 1      /* infl == OCCUPIED makes a voxel OCC too */
#define MLM_OCT_OCC_ONLY 2  /* FREE voxels count as NONE */
#define MLM_OCT_ROW 40      /* int64 in summary */
int mlm_export_octree(mlm_handle *h, const int32_t lo[3], const int32_t dims[3], int depth, int flags, uint16_t *words,
                      int32_t *inner4, int32_t *skip, int64_t cap_inner, int32_t *leaf4, int8_t *leaf_class, int64_t cap_leaves,
                      int64_t summary[MLM_OCT_ROW]);
/* Load blocks into the map (no reference counterpart: the reference never persists or merges maps; this is how a
 * merged global map, mlmapping_amd/merge.py, is put back behind the query interface).  keys [n*3]; log_odds / occ /
 * infl [n*cells] and collapsed [n] as mlm_export_blocks / mlm_export_block_flags write them, any of them may be NULL
 * (that plane keeps its current content; new blocks start as allocate_ram leaves them: 0 / 'u' / 'u'); sources may
 * be host or device memory.  Blocks already present are overwritten cell by cell, others are created. */
int mlm_import_blocks(mlm_handle *h, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ,
                      const uint8_t *infl, const uint8_t *collapsed);

/* Make the map smaller, in place on the device: drop — or page out — the blocks of a box of block KEYS (no reference counterpart:
 * the reference's observed_group_map only ever grows, and so did the pool here; a vehicle that keeps flying ends with
 * MLM_ERR_CAPACITY).  The box is in block keys — the glb_id of mlm_query_odds_at, the keys of mlm_export_blocks — not in voxels: a
 * block is inside iff key_lo[a] <= key[a] < key_lo[a] + key_dims[a] on all three axes.  MLM_CROP_OUTSIDE drops the blocks outside the
 * box (keep a window), MLM_CROP_INSIDE those inside it.  A dropped block is gone as if it had never been created: every query and
 * read-out answers for its voxels what it answers for an absent block, a later frame that reaches it creates it afresh (allocate_ram);
 * in frontier mode its frontier flags and its released / observed flags go with it, frontier cells of kept blocks stay.
 *   Outputs (each may be NULL; cap blocks each, in the layout of mlm_export_blocks / mlm_export_block_flags; device memory of this
 * device is written in place, any host memory is staged): the dropped blocks in ascending order of their old slot — what
 * mlm_import_blocks takes to bring them back later.  collapsed is 0 outside frontier mode.  With any output given and cap smaller than
 * the number of dropped blocks: MLM_ERR_CAPACITY, the map untouched, summary filled so the caller can size.  With no output, cap is
 * ignored and the blocks are just dropped.
 *   summary (may be NULL): [0] blocks before, [1] kept K, [2] dropped D, [3] dropped blocks written, [4] block capacity before,
 * [5] after, [6] mlm_frame_stats.device_bytes before, [7] after.  MLM_CROP_DRY only counts: summary is filled, the map is not touched.
 *   The pool is compacted in place by hole filling (mlmapping_amd/csrc/mlm_crop.h): with d(s) the number of dropped slots below slot
 * s and H = d(K), the h-th dropped slot below K takes the h-th kept slot at or above K; at most min(D, K) blocks move, the kept blocks
 * below K stay where they are, and mlm_export_blocks' raw order afterwards is that one answer.  D == 0 changes nothing at all.
 *   MLM_CROP_SHRINK afterwards gives pool memory back: with c0 the capacity mlm_create gave the pool, the target is the smallest
 * c0 * 2^k >= max(c0, 2 K); if that is below the current capacity the K blocks move into a pool of that size.  Best effort: if the
 * smaller pool cannot be allocated next to the current one the crop still stands and summary[5] reports the unchanged capacity; ignored
 * with the knob "pool_grow" = 0.
 *   Like mlm_import_blocks the call waits for everything submitted first.  MLM_ERR_INVALID (with a text in mlm_last_error): a NULL box,
 * a dim < 1, key_lo + key_dims beyond int32, an unknown flag bit, cap < 0.  Every check, the count and every allocation come before
 * the first write into the pool: a failing call leaves the map as it was. */
enum { MLM_CROP_OUTSIDE = 0,  /* drop the blocks whose key lies outside the box: keep a window */
       MLM_CROP_INSIDE  = 1,  /* drop the blocks whose key lies inside the box */
       MLM_CROP_DRY     = 2,  /* count only: summary is filled, the map is not touched */
       MLM_CROP_SHRINK  = 4 };/* afterwards give pool memory back (rule above) */
#define MLM_CROP_ROW 8
int mlm_crop_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int flags, int cap,
                    int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, uint8_t *collapsed,
                    int64_t summary[MLM_CROP_ROW]);

/* Resample the map under a rigid transform: the map's voxel content written onto the lattice of another frame, as blocks in the layout
 * mlm_import_blocks and the merge take (no reference counterpart: the reference's map lives in one frame for good).  What a pose
 * correction (mlm_score_poses), a merge of maps whose origins differ, or blocks paged out before the odometry frame was corrected need.
 *   T_sd: 12 doubles as in mlm_score_poses / mlm_render_depth (R row major, then o); it maps a point of the DESTINATION (new) frame to
 * the SOURCE (current map) frame and is never inverted for the values.  The answer is defined per destination voxel v = g * subbox_n + c
 * (block key g, cell coordinate c), in IEEE double, nothing fused (mlmapping_amd/csrc/mlm_warp.h):
 *     centre   p_a = (g_a * d_glb + c_a * d_sub) + d_sub_half                (subbox_id2xyz_glb_vec);
 *     source   w_a = ((R[a][0] * p_0 + R[a][1] * p_1) + R[a][2] * p_2) + o_a  (mlm_score_poses' rule);
 *     voxel    floor((w_a / d_sub) * 1024) >> 10, invalid if a lattice value is not finite or beyond 2^40; block and cell by floor division.
 * The voxel is LIVE iff the lattice step is valid, the source block's key lies inside the 21-bit key range and the block is present, and
 * — with MLM_WARP_SEEN — the source voxel's occ != 'u' or its infl == 'o'.  A live voxel takes the source voxel's raw log_odds, occ and
 * infl (a released block answers from element 0 with infl 'u', as the queries do); every other voxel is 0.0f / 'u' / 'u', what
 * allocate_ram leaves.  Nearest voxel only: classes and log-odds stay consistent with each other and the result is exact.
 *   A destination block is EMITTED iff it holds at least one live voxel, its key lies inside the 21-bit range and inside the key box
 * (key_lo / key_dims: mlm_crop_blocks' box semantics; both NULL: no restriction).  The emitted blocks are written in ascending order
 * of their packed key — x, then y, then z — into keys [cap*3], log_odds / occ / infl [cap*cells]; each may be NULL; device memory of
 * this device is written in place, any host memory is staged.  With an output given and cap smaller than the number of emitted
 * blocks: MLM_ERR_CAPACITY, nothing written but summary.  MLM_WARP_DRY only counts.
 *   summary (may be NULL): [0] source blocks, [1] candidate blocks examined (an implementation count >= [2]), [2] emitted blocks E,
 * [3] blocks written, [4] live voxels, [5] / [6] live voxels with occ 'o' / 'f', [7] live voxels with infl 'o'.
 *   MLM_WARP_REPLACE: afterwards the handle holds the warped map instead of its own — exactly what "this call into device buffers, drop
 * every block (mlm_crop_blocks, MLM_CROP_INSIDE, an all-covering box), mlm_import_blocks of the dump" does on the same handle, and made
 * of those code paths.  Frame slots, graphs and container state survive as across a crop.  Every check, the count and every allocation
 * come before the first write into the pool: a failing call leaves the map as it was.  Refused (MLM_ERR_INVALID) on a frontier-mode
 * handle: frontier and released flags have no resampled meaning.  Without it the call only reads the map, frontier mode included.
 *   Like mlm_import_blocks the call waits for everything submitted first.  MLM_ERR_INVALID (with a text in mlm_last_error): a NULL
 * T_sd, a non-finite entry, max |R R^T - I| > 1e-9 (the transform must be rigid), one of key_lo / key_dims NULL and the other not,
 * mlm_crop_blocks' box errors, an unknown flag bit, cap < 0. */
enum { MLM_WARP_SEEN    = 1,  /* only voxels the source map has observed (occ != 'u') or inflated (infl == 'o') are live */
       MLM_WARP_REPLACE = 2,  /* afterwards the handle holds the warped map */
       MLM_WARP_DRY     = 4 };/* count only: summary is filled, nothing is written */
#define MLM_WARP_ROW 8
int mlm_warp_blocks(mlm_handle *h, const double T_sd[12], const int32_t key_lo[3], const int32_t key_dims[3],
                    int flags, int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl,
                    int64_t summary[MLM_WARP_ROW]);

/* Fuse a block dump into the live map, in place on the device — or, with MLM_FUSE_DRY, only compare the two (no reference counterpart:
 * the reference has one map).  What pages a region back in without destroying what was integrated there since (mlm_import_blocks
 * overwrites whole blocks), loads another handle's or another robot's map after mlm_warp_blocks has put it on this lattice, and answers
 * "where do these two maps disagree".  keys [n*3], log_odds / occ / infl [n*cells] as mlm_export_blocks, mlm_crop_blocks and
 * mlm_warp_blocks write them; each pointer on its own may be host or device memory (host memory is staged); infl, per_row and summary
 * may be NULL; summary is host memory, per_row host or device memory.  Rows are full blocks: there is no collapsed input (a dump of a
 * frontier-mode handle is made with mlm_warp_blocks, which expands released blocks).
 *   The rule per voxel (mlmapping_amd/csrc/mlm_fuse.h), IEEE single, nothing fused.  The map holds (La, occ_a, infl_a) — 0.0f / 'u' / 'u'
 * where it has no block —, the dump (Lb, occ_b, infl_b); clamp(x) = !(x >= log_odds_min) ? log_odds_min : (x > log_odds_max ?
 * log_odds_max : x), so a NaN becomes log_odds_min; Lb' = clamp(Lb).  The voxel CONTRIBUTES iff occ_b is 'f' or 'o'; seen_a = occ_a != 'u'.
 * A contributing voxel is WRITTEN always in MLM_FUSE_ADD, MAX and TAKE, in MLM_FUSE_FILL iff !seen_a, with
 *     ADD: L = La + Lb'      MAX: L = seen_a ? (La > Lb' ? La : Lb') : Lb'      TAKE, FILL: L = Lb'
 * log_odds = clamp(L) and occ = clamp(L) > occupied_sh ? 'o' : 'f' — mlm_merge_finish's rule, not the integrate path's hysteresis.  A
 * voxel that is not written keeps its log-odds and its class bit for bit.  With infl given and infl_b == 'o', infl_a becomes 'o', in
 * every mode and whether or not the voxel contributes; otherwise infl_a is unchanged.
 *   Blocks.  Row r TOUCHES iff it has a contributing voxel, or infl is given and it has a voxel with infl_b == 'o'.  A touching row
 * whose block is absent creates it; the created blocks take the slots n_blocks_before + rank, rank = the number of created rows with a
 * smaller row index (a prefix sum, not a race for a counter), so mlm_export_blocks' raw order afterwards is one answer, as it is after
 * mlm_crop_blocks.  An absent row that touches nothing creates nothing; a present row that touches nothing changes nothing.
 *   summary — all counts, one value whatever the schedule: [0] rows, [1] rows whose block the map held, [2] rows created, [3] rows that
 * touch nothing, [4] contributing voxels, of those [5] with !seen_a, [6] both seen and occ_a == occ_b, [7] both seen and occ_a != occ_b
 * (the conflicts; [4] == [5] + [6] + [7]), [8] voxels whose class is 'o' afterwards and was not before, [9] voxels whose class was 'o'
 * and is 'f' afterwards, [10] voxels whose infl turned 'o', [11] voxels whose log-odds bits changed.
 *   per_row [n][MLM_FUSE_COLS]: [0] contributing voxels of the row, [1] its conflicts, [2] its share of [8] + [9], [3] 0 block present,
 * 1 created, 2 absent and left absent.
 *   MLM_FUSE_DRY fills summary and per_row as the call without it would ([2] and per_row[3] == 1: would be created) and touches
 * nothing: no block is created, no pool grows, the host mirror stays valid — the map diff.
 *   Frontier mode: without MLM_FUSE_DRY the call is refused (MLM_ERR_INVALID), for mlm_warp_blocks' MLM_WARP_REPLACE's reason; with it a
 * released block answers from element 0 with infl 'u', as mlm_merge_pack and the queries read it.
 *   Like mlm_import_blocks the call waits for everything submitted first.  MLM_ERR_INVALID (with a text in mlm_last_error): n < 0;
 * keys, log_odds or occ NULL with n > 0; a mode outside 0..3; an unknown flag bit; a key outside the 21-bit key range [-2^20, 2^20);
 * two rows with the same key.  n == 0: MLM_OK, a zero summary.  MLM_ERR_CAPACITY: the pool cannot take the created blocks (knob
 * "pool_grow" = 0, or no device memory), or no memory for the staging.  Every check, every count and every allocation — pool growth,
 * staging, the handle's scratch (counted in device_bytes) — come before the first write into pool or hash table: a failing call leaves
 * the map byte for byte as it was. */
enum { MLM_FUSE_ADD = 0, MLM_FUSE_MAX = 1, MLM_FUSE_TAKE = 2, MLM_FUSE_FILL = 3 };  /* mode */
enum { MLM_FUSE_DRY = 1 };                                                          /* flags */
#define MLM_FUSE_ROW 12   /* int64 in summary */
#define MLM_FUSE_COLS 4   /* int32 per row of per_row */
int mlm_fuse_blocks(mlm_handle *h, int n, const int32_t *keys, const float *log_odds, const uint8_t *occ,
                    const uint8_t *infl, int mode, int flags, int32_t *per_row, int64_t summary[MLM_FUSE_ROW]);

/* Age the map, in place on the device: decay the log-odds of the selected blocks towards zero, optionally forget voxels whose evidence
 * has become small, and optionally drop the blocks that are empty afterwards (no reference counterpart: the reference's
 * observed_group_map only ever accumulates evidence).  One pass over the planes of the selected blocks: 6 bytes read and at most 6
 * written per voxel, no sum over floats.
 *   Selection.  key_lo / key_dims are mlm_crop_blocks' box of block keys, with its checks and error texts; both NULL selects every block
 * (MLM_AGE_OUTSIDE or not).  A block is SELECTED iff its key lies inside the box — with MLM_AGE_OUTSIDE iff it lies outside it ("age
 * everything but where the sensor is looking").  A voxel of a block that is not selected keeps all three planes bit for bit.
 *   The rule per voxel (La, occ_a, infl_a) of a selected block (mlmapping_amd/csrc/mlm_age.h), IEEE single, nothing fused, subnormals
 * kept; clamp is mlm_fuse_blocks' (a NaN becomes log_odds_min).  The voxel is AGED iff occ_a != 'u' or (bits(La) & 0x7fffffff) != 0: it
 * holds a class or evidence (a hit below occupied_sh leaves occ 'u' with nonzero log-odds); allocate_ram's 0.0f / 'u' and a -0.0f are
 * not aged and keep their bits.  For an aged voxel
 *     MLM_AGE_SCALE: L = La * amount      MLM_AGE_STEP: L = La > amount ? La - amount : (La < -amount ? La + amount : 0.0f)
 * (towards zero, never across it), then L = clamp(L).  With MLM_AGE_FORGET and fabsf(L) <= forget the voxel is FORGOTTEN: log-odds
 * +0.0f, occ 'u'.  Otherwise, if occ_a != 'u', occ = L > occupied_sh ? 'o' : 'f' — mlm_fuse_blocks' and mlm_merge_finish's rule, not
 * the integrate path's hysteresis — and if occ_a == 'u' occ stays 'u': evidence that never reached a class decays, aging never
 * classifies.  Log-odds = L.  infl is untouched, except with MLM_AGE_CLEAR_INFL, which sets the infl of EVERY voxel of a selected block
 * to 'u', aged or not (a halo whose obstacle was forgotten is stale; the caller runs mlm_inflate_map again afterwards).
 *   Empty blocks.  A selected block is EMPTY afterwards iff every voxel of it has occ 'u', infl other than 'o' and (bits(L) &
 * 0x7fffffff) == 0.  With MLM_AGE_DROP the empty selected blocks — those that were empty before the call included — are dropped exactly
 * as mlm_crop_blocks drops blocks: its hole-filling rule over that drop set, so mlm_export_blocks' raw order afterwards is one answer
 * whatever the schedule; hash table, block count, mlm_frame_stats.n_blocks and the host mirror follow; frame slots, graphs and
 * container state survive as across a crop.  Nothing is paged out and no pool memory is given back: a caller who wants that calls
 * mlm_crop_blocks (MLM_CROP_SHRINK) afterwards.
 *   summary (host memory, may be NULL) — all counts, one value whatever the schedule: [0] blocks before, [1] selected blocks, [2] blocks
 * dropped, [3] blocks afterwards, [4] aged voxels, [5] voxels whose log-odds bits changed, [6] forgotten voxels, of those [7] with class
 * 'o' and [8] with class 'f' ([6] - [7] - [8]: evidence only), [9] voxels 'o' -> 'f', [10] voxels 'f' -> 'o' (a negative occupied_sh),
 * [11] voxels whose infl went 'o' -> 'u'.
 *   per_block [blocks before][MLM_AGE_COLS] (host or device memory, or NULL; host memory is staged), indexed by the OLD slot: [0] aged
 * voxels, [1] forgotten voxels, [2] the block's share of [9] + [10], [3] 0 not selected, 1 selected and kept, 2 selected and dropped —
 * with MLM_AGE_DRY or without MLM_AGE_DROP 2 reads "empty, would be dropped".
 *   MLM_AGE_DRY fills summary and per_block as the call without it would and touches nothing: no plane, no pool, the host mirror stays
 * valid.  Like mlm_import_blocks the call waits for everything submitted first.  MLM_ERR_INVALID (with a text in mlm_last_error): one of
 * key_lo / key_dims NULL and the other not, mlm_crop_blocks' box errors, an unknown flag bit, a mode outside 0..1, a non-finite amount,
 * MLM_AGE_SCALE with amount outside [0, 1], MLM_AGE_STEP with amount < 0, MLM_AGE_FORGET with a non-finite or negative forget (without
 * the flag forget is ignored), a frontier-mode handle, dry or not (frontier, released and observed flags have no aged meaning:
 * MLM_WARP_REPLACE's reason).  Zero blocks: MLM_OK, a zero summary.  Every check and every allocation — the handle's scratch (counted
 * in device_bytes), the staging of a host per_block — come before the first write into the pool: a failing call leaves the map byte
 * for byte as it was. */
enum { MLM_AGE_SCALE = 0, MLM_AGE_STEP = 1 };                       /* mode */
enum { MLM_AGE_OUTSIDE = 1, MLM_AGE_DRY = 2, MLM_AGE_FORGET = 4,
       MLM_AGE_DROP = 8, MLM_AGE_CLEAR_INFL = 16 };                  /* flags */
#define MLM_AGE_ROW 12   /* int64 in summary */
#define MLM_AGE_COLS 4   /* int32 per block of per_block */
int mlm_age_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3], int mode, float amount, float forget,
                   int flags, int32_t *per_block, int64_t summary[MLM_AGE_ROW]);

/* Which blocks differ from the last time the caller looked: a digest of 16 bytes per block, and — against the digest table an earlier
 * call wrote — the blocks whose content differs, the blocks that are new and the keys that are gone (no reference counterpart: the
 * reference hands its whole map out every time).  The call only reads the map: frontier-mode handles are accepted, the host mirror
 * stays valid.  One pass over the planes of the selected blocks: 6 bytes read per voxel.
 *   Selection.  key_lo / key_dims are mlm_crop_blocks' box of block keys, with its checks and error texts; both NULL selects every
 * block.  A block of the map is SELECTED iff its key lies inside the box.  Rows of the previous table outside the box are ignored:
 * neither compared, nor reported gone, nor copied into the new table.
 *   The view of a block: its `cells` triples (log-odds bits, occ, infl) as mlm_warp_blocks reads them — a released block of a
 * frontier-mode handle answers from element 0 with infl 'u' in every cell; with MLM_DELTA_NO_INFL infl is 'u' everywhere.
 *   The digest (mlmapping_amd/csrc/mlm_delta.h): two uint64 per block, arithmetic mod 2^64, over the cell index c = 0 .. cells - 1:
 *     w_c  = bits(L_c) | (uint64)occ_c << 32 | (uint64)infl_c << 40
 *     x_c  = w_c ^ ((c + 1) * 0x9E3779B97F4A7C15)
 *     f(x) : x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *     d[0] = sum_c f(x_c)            d[1] = sum_c f(x_c ^ 0xD6E8FEB86659FD93)
 * A sum of integers: one value whatever the schedule, no atomic and no float.  It is over the bits, so -0.0f and +0.0f differ.
 * "Changed" means the 128 bits differ.  A changed block is missed with probability about 2^-128 per comparison.  The digest is not
 * secure against someone constructing collisions.
 *   The tables.  prev_keys [n_prev*3] and prev_digest [n_prev*2] are the table an earlier call wrote: keys strictly ascending by
 * packed key (x, then y, then z, each biased by 2^20) and inside the 21-bit range; n_prev == 0 means "everything is new".  cur_keys
 * [cap_table*3] and cur_digest [cap_table*2] receive the S selected blocks in the same ascending order: a valid prev of the next call.
 *   The join.  A selected block is UNCHANGED (its key is in prev with an equal digest), CHANGED (in prev with a different digest) or
 * NEW (not in prev).  A prev row inside the box whose key the map does not hold is GONE.
 *   Emitted blocks: the CHANGED and the NEW ones together, ascending by packed key — keys [cap*3] and the view's planes log_odds / occ
 * / infl [cap*cells] in the layout mlm_import_blocks takes (a released block expanded, infl 'u' throughout with MLM_DELTA_NO_INFL),
 * kind [cap] 1 changed / 2 new.  gone_keys [cap_gone*3], ascending.  Every output pointer may be NULL; each input or output pointer
 * on its own may be host memory or memory of this device (host memory is staged); summary is host memory.
 *   summary — all counts: [0] blocks in the map, [1] selected S, [2] n_prev, [3] prev rows inside the box P, [4] unchanged, [5] changed
 * C, [6] new N, [7] gone G, [8] blocks written, [9] table rows written, [10] gone keys written, [11] selected blocks that are empty by
 * mlm_age_blocks' predicate on the planes as they are (is an MLM_AGE_DROP worth it?).  S = [4] + C + N and P = [4] + C + G.
 *   MLM_DELTA_DRY fills summary and writes nothing else.  Like mlm_import_blocks the call waits for everything submitted first.
 * MLM_ERR_INVALID (with a text in mlm_last_error; no output is written, summary included): mlm_crop_blocks' box errors, one of key_lo
 * / key_dims NULL and the other not, an unknown flag bit, a negative cap or n_prev, n_prev > 0 with a NULL prev pointer, a prev key
 * outside the 21-bit range, prev keys not strictly ascending (the last two are found on the device).  MLM_ERR_CAPACITY if a given
 * output's cap is below its count (cap_table < S with cur_keys or cur_digest given, cap < C + N with a block output given, cap_gone
 * < G with gone_keys given): nothing is written but summary, so the caller can size.  An empty map with no previous table: MLM_OK
 * and a summary of counts only.  Scratch is kept by the handle and counted in device_bytes; every allocation comes before the first
 * store to a caller's buffer. */
enum { MLM_DELTA_DRY = 1,       /* count only: summary is filled, nothing else is written */
       MLM_DELTA_NO_INFL = 2 }; /* infl reads as 'u' in the digest and is not emitted as a difference */
#define MLM_DELTA_ROW 12
int mlm_delta_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3],
                     int n_prev, const int32_t *prev_keys, const uint64_t *prev_digest, int flags,
                     int cap_table, int32_t *cur_keys, uint64_t *cur_digest,
                     int cap, int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, uint8_t *kind,
                     int cap_gone, int32_t *gone_keys, int64_t summary[MLM_DELTA_ROW]);

/* A lossless packed block stream, and back (no reference counterpart).  The block dump costs 12 bytes of key and 6 bytes per voxel
 * whatever a block holds; the stream uses what is regular in a map — occ and infl hold one of three bytes, unseen voxels are +0.0f,
 * long-observed ones sit exactly on log_odds_min or log_odds_max — and nothing else: every bit comes back.  One byte string per input,
 * whatever the schedule.  mlm_pack_blocks only reads the map: frontier-mode handles are accepted, the host mirror stays valid.
 *   The stream, little endian.  C = subbox_n^3 cells per block, W = ceil(C / 64).  A PLANE is W uint64: bit i of word j belongs to cell
 * 64 j + i, bits of cells >= C are zero.
 *     header, 64 bytes:  0 "MLMPACK1" | 8 u32 C | 12 u32 subbox_n | 16 u32 n blocks | 20 u32 flags (bit 0: infl was left out) | 24 u32
 *                        bits of (float)log_odds_min | 28 u32 bits of (float)log_odds_max | 32 u64 total bytes of the stream | 40 u64
 *                        literals in the stream | 48..63 zero
 *     directory, 16 bytes per block in row order: int32 key[3] | u32 offset of the block's record in 8-byte units from the start
 *     records, back to back in row order behind the directory, each 8-byte aligned: u32 presence (bits 0..5) | u32 n_lit | the present
 *                        planes in the order occ0 occ1 infl0 infl1 val0 val1 | n_lit uint32 literals | zero padding to 8 bytes
 *   Codes per cell.  occ and infl: 'u' 0, 'f' 1, 'o' 2 — bit 0 in plane 0, bit 1 in plane 1; code 3 never occurs.  val, decided on the
 * log-odds BITS in this order: 0 if they are zero, 1 if they equal the header's lo_min bits, 2 if they equal its lo_max bits, 3
 * otherwise; a code-3 cell appends its 32 bits to the literals, in cell order (so -0.0f, NaNs and subnormals survive as bits).  The
 * encoder writes a plane iff it has a set bit (the canonical stream); a blank block (+0.0f / 'u' / 'u' throughout) is 8 bytes of
 * record and its directory row.
 *   mlm_pack_blocks.  keys == NULL packs the live map: the blocks of the key box key_lo / key_dims (mlm_delta_blocks' box, with its
 * checks and texts; both NULL: every block) in ascending packed-key order, each seen through mlm_delta_blocks' view (a released block
 * of a frontier-mode handle expanded); n is ignored; the call waits for everything submitted first.  keys != NULL packs n rows of a
 * dump in the layout mlm_import_blocks takes, in row order (the box must be NULL; infl == NULL reads as 'u'; each pointer on its own
 * host memory or memory of this device).  MLM_PACK_NO_INFL: infl reads 'u', header flag bit 0 is set.  MLM_PACK_DRY, or a NULL stream:
 * only the summary.  stream [cap_bytes] is host memory (staged) or 8-byte-aligned device memory.
 *   summary: [0] blocks, [1] stream bytes, [2] raw bytes n (12 + 6 C), [3] blank blocks, [4] literals, [5] cells coded lo_min, [6]
 * cells coded lo_max, [7] bytes written.
 *   MLM_ERR_INVALID (a text in mlm_last_error, nothing written): the box errors, a box together with rows, a negative n, rows without
 * log_odds or occ, an unknown flag, a misaligned device stream, an occ or infl byte outside 'u' 'f' 'o' (found on the device; the text
 * names the row).  MLM_ERR_CAPACITY with the summary filled: cap_bytes below [1], or a stream beyond 2^32 - 1 eight-byte units.  Every
 * check, the sizes, the prefix and every allocation come before the first store to stream.  Scratch is kept by the handle and counted
 * in device_bytes.
 *   mlm_unpack_blocks writes the rows mlm_import_blocks, mlm_fuse_blocks and mlm_warp_blocks' consumers take: keys [cap*3], log_odds
 * / occ / infl [cap*cells], each NULL, host or device memory; all NULL only sizes (summary[0] blocks).  lo_min / lo_max come from
 * the stream's header, not from the handle.  The whole stream is validated before the first store, no byte beyond `bytes` is read, and
 * any byte content gets a verdict.  MLM_ERR_INVALID with the check's number in the text: 1 bytes below the header, 2 a wrong magic, 3
 * C or subbox_n not the handle's, 4 the header's total above bytes (or below header + directory), 5 a directory offset that is not
 * exactly the previous record's end (the first: (64 + 16 n) / 8), 6 presence >= 64, 7 a set bit for a cell >= C, 8 an occ or infl code
 * 3, 9 n_lit other than the popcount of val0 & val1, 10 a record running past the total (or the last one ending short of it); 11 .. 14
 * the arguments (a NULL stream, a flag — none is defined —, a negative cap, a misaligned device stream).  The verdict is the failure with
 * the smallest (block, check).  MLM_ERR_CAPACITY if cap < n with an output given.  summary as above, [7] the bytes written to the
 * outputs. */
enum { MLM_PACK_DRY = 1,       /* size only: summary is filled, nothing else is written */
       MLM_PACK_NO_INFL = 2 }; /* infl reads as 'u' and the header says so */
#define MLM_PACK_ROW 8
int mlm_pack_blocks(mlm_handle *h, const int32_t key_lo[3], const int32_t key_dims[3],
                    int n, const int32_t *keys, const float *log_odds, const uint8_t *occ, const uint8_t *infl,
                    int flags, size_t cap_bytes, void *stream, int64_t summary[MLM_PACK_ROW]);
int mlm_unpack_blocks(mlm_handle *h, const void *stream, size_t bytes, int flags, int cap,
                      int32_t *keys, float *log_odds, uint8_t *occ, uint8_t *infl, int64_t summary[MLM_PACK_ROW]);

/* The two device-side steps of the optional global-map merge across GPUs (mlmapping_amd/merge.py; no reference
 * counterpart: SURVEY.md §8e).  All pointers are device memory; both calls return when the buffers are written.
 * pack:   row b of log_odds_dev / seen_dev [n*cells] = this map's cells of block keys_dev[3b..3b+2] (0 / 0 where the
 *         map does not hold the block; seen = occupancy != 'u').  These rows are what the ranks exchange and sum.
 * finish: summed log-odds clamped to [log_odds_min, log_odds_max]; occ = 'o' above occupied_sh, else 'f' where any
 *         rank had seen the voxel, else 'u'. */
int mlm_merge_pack(mlm_handle *h, const int32_t *keys_dev, int n, float *log_odds_dev, uint8_t *seen_dev);
int mlm_merge_finish(mlm_handle *h, float *log_odds_dev, const uint8_t *seen_dev, size_t n_cells, uint8_t *occ_dev);

/* Pin a caller-owned host buffer (hipHostRegister) so that the host-buffer entry points (mlm_integrate_depth_batch,
 * mlm_integrate_depth_u16, mlm_integrate_callback, mlm_integrate_points) DMA straight from it: from pageable memory a copy is
 * staged by the HIP runtime at a third of the link's rate.  A replay tool registers its frame buffer once; the ROS callback
 * pattern (one frame per call) does not need it.  Registering does not change the lifetime rule: every entry point is done with
 * the buffer when it returns (see mlm_set_async).  Unregister before freeing the buffer (waits for everything submitted). */
int mlm_host_register(mlm_handle *h, const void *ptr, size_t bytes);
int mlm_host_unregister(mlm_handle *h, const void *ptr);

int mlm_sync(mlm_handle *h);
/* async = 1: integrate calls return once the work is SUBMITTED (up to three batches may be in flight, one per slot set); errors of
 * a batch and mlm_get_frame_stats lag by one call; mlm_sync, queries and exports wait for everything.  Default 0: integrate
 * calls return when the map is updated (a lone frame's call returns on a completion ticket its last map-updating kernel writes to pinned
 * memory; in frontier mode the release scan of map_local.cpp:208-232 — which marks blocks, not voxels — may still be running then:
 * everything that reads the map afterwards is ordered behind it).  Host buffers stay BORROWED FOR THE CALL in both modes: an asynchronous call returns
 * only after its copies out of the caller's buffer have completed (also from a buffer pinned with mlm_host_register, whose
 * copies are truly asynchronous) — the buffer may be refilled as soon as the call returns.  Device inputs of the *_dev entry
 * points are read by the frames' kernels and must stay unmodified until mlm_sync (or until three further batches were submitted).
 * A call whose frames leave the sector path (a fall-back, a frame too wide for it) runs them one by one and returns once they are applied. */
int mlm_set_async(mlm_handle *h, int on);
/* Small query batches (a planner asking position by position, include/mlmap.h:170-295) are answered from a pinned HOST copy of the
 * block planes (6 bytes per voxel + 13 per block), which grows with the map.  max_bytes bounds that pinned memory (default 1 GiB;
 * 0, or less than the copy's smallest size of 256 blocks: no host copy at all): a map that needs more is queried by kernels only, as
 * large batches always are — same answers, ~20 us per call instead of ~0.05 us; the query that finds the map grown beyond the limit
 * is one of them.  Lowering the limit below what is pinned frees the copy; raising it again brings the copy back at the next query. */
int mlm_set_host_mirror_limit(mlm_handle *h, size_t max_bytes);
int mlm_get_frame_stats(mlm_handle *h, mlm_frame_stats *out);

/* test hooks (need limits.record_awareness): unique hit cells (linear cell idx, odd, first-touch time) and
 * unique miss cells of the LAST frame, unordered */
int mlm_get_awareness_hits(mlm_handle *h, int cap, uint32_t *cell_idx, float *odds, uint32_t *t_first, int *n_out);
int mlm_get_awareness_misses(mlm_handle *h, int cap, uint32_t *cell_idx, int *n_out);
/* derived constants, for cross-checking against the oracle: T_ls of the last frame, odds table [21*n_rho] */
int mlm_get_T_ls(mlm_handle *h, double q[4], double t[3]);
int mlm_get_odds_table(mlm_handle *h, float *out);

/* Device time of the launches of the integrate calls, measured with HIP events on the streams the kernels run on
 * (milliseconds); names are static strings.  on = 1: the list describes the last call only; on = 2: it accumulates over
 * calls until read (mlm_get_kernel_times with cap >= n consumes it); on = 3: like 2 but only every `every`-th
 * launch of ONE kernel is bracketed (mlm_set_timed_kernel, default "k_bin_points", 1; events around every kernel cost
 * ~19 % throughput) — bench.py uses 2 on a few batches to find the dominant kernel and 3 on it over its timed region; on = 4: only the spans of a batch's Stage A and Stage B+C ("stage_a_batch",
 * "stage_bc_batch"; the latter starts when the main stream reaches it, i.e. after the previous batch's).
 * Stage A kernels are launched once per batch, so one entry of theirs covers all frames of that batch. */
int mlm_get_kernel_times(mlm_handle *h, int cap, const char **names, float *ms, int *n_out);
int mlm_enable_kernel_timing(mlm_handle *h, int on);
int mlm_set_timed_kernel(mlm_handle *h, const char *name, int every);

/* Test and experiment knobs — NOT part of the drop-in contract.  Named integers read by the NEXT mlm_create of this process:
 * forced fall-backs ("sec_fail_every", "sec_backoff", "sectors"), a fixed pool ("pool_grow"), slot layout ("slot_sets"), launch
 * geometries ("sec_tab", "sec_threads", "rank_grid", ...; the full
 * list is kKnobNames in mlmapping_amd/csrc/mlm_handle.h).  Unknown names: MLM_ERR_INVALID.  mlm_debug_reset forgets them all.  The library reads
 * no environment variable for behaviour; MLM_DEBUG_CREATE / MLM_DEBUG_ALLOC / MLM_DEBUG_DRAIN only print diagnostics. */
int mlm_debug_set(const char *name, long long value);
int mlm_debug_reset(void);
/* Host clocks of the synchronous single-frame path of mlm_integrate_callback (a development aid, like the knobs): microseconds
 * summed over the calls since the last reset — [0] pose compensation, drain of the previous call, sampling; [1] frame set-up up
 * to the launch; [2] the launch call (hipGraphLaunch); [3] host work between launch and wait; [4] waiting for the frame's ticket;
 * [5] the rest of the call. */
int mlm_debug_clocks(mlm_handle *h, double out_us[8], int reset);
/* Test hook for the binning kernel's cheap arithmetic (mlm_bin_point_fast, mlm_device.h): the largest relative errors, over 2^26
 * values, of the hardware's reciprocal and reciprocal-square-root seeds [0], [2] and of their once-refined forms [1], [3] — the
 * error budget of the certified margins assumes [1], [3] <= 4e-12. */
int mlm_debug_probe_seeds(mlm_handle *h, double out4[4]);

#ifdef __cplusplus
}
#endif
#endif
