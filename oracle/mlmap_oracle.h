/*
 * mlmap_oracle.h — C ABI of the CPU oracle.
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load this library.  The product path
 * (mlmapping_amd/, include/mlmap_hip.h) never links, imports or calls it.
 *
 * The oracle is a CPU restatement of the reference's per-frame map update
 * (mlmap::update_map = awareness_map_cylindrical::input_pc_pose +
 * local_map_cartesian::input_pc_pose_direct) and of the mlmap.h query inlines.
 * Every function in mlmap_oracle.cpp cites the reference file:line it follows.
 *
 * PARITY PINNING STATUS: "parity unpinned" in the strict sense of the task rules —
 * the reference ships no first-party tests, golden vectors or fixtures for this path
 * (SURVEY.md §4), and it cannot be compiled here without writing stand-in headers for
 * Eigen / PCL / ROS (forbidden), so no oracle/_ref build exists.  What pins the oracle
 * instead: the known-answer counts recorded in SURVEY.md §8d (hit/miss/block/'o'/'f'
 * cell counts for configs 1, 3 and the reference-default sampler case, including the
 * iteration-order dependent frame-19 counts), reproduced by tests/test_oracle_kat.py, and
 * the property tests the reference holds for Sophus (test_so3.cpp, test_se3.cpp), to which
 * tests/test_host_math.py holds the SO3 / SE3 restatements below.
 */
#ifndef MLMAP_ORACLE_H
#define MLMAP_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Same field meaning as the YAML keys read at mlmap.cpp:10-33,75-85. */
typedef struct mlo_config {
    /* awareness map (map_awareness.cpp:19) */
    double am_d_rho;
    double am_d_phi_deg;
    double am_d_z;
    int32_t am_n_rho;
    int32_t am_n_z_below;
    int32_t am_n_z_over;
    int32_t use_raycasting;
    double depth_noise_coe;
    /* local map (map_local.cpp:46) — doubles are cast to float exactly as mlmap.cpp:77-81 */
    double subbox_d_xyz;
    int32_t subbox_n;
    int32_t use_exploration_frontiers;
    double log_odds_min;
    double log_odds_max;
    double measurement_hit;
    double measurement_miss;
    double occupied_sh;
    /* inflation (mlmap.cpp:10,84-85; map_local.h:63-65) */
    int32_t inflate_n;
    int32_t inflate_global_n;
    int32_t apply_inflate;
    int32_t sample_cnt; /* mlmapping_sample_cnt (mlmap.cpp:14) */
    /* pinhole intrinsics; stored as float like mlmap.h:92 */
    double cam_cx, cam_cy, cam_fx, cam_fy;
    /* T_B_S, 4x4 row major (yamlRead.h:16-24) */
    double T_bs[16];
} mlo_config;

typedef struct mlo_handle mlo_handle;

/* process-wide: 0 = Eigen's generic quaternion product / norm (default), 1 = the association of Eigen's SSE2 double kernels
 * (see mlmap_oracle.cpp: quat_mul) — a sensitivity switch for the one piece of third-party arithmetic on the path */
void mlo_set_quat_arch(int arch);
mlo_handle *mlo_create(const mlo_config *cfg);
void mlo_destroy(mlo_handle *h);

/* One mlmap::update_map() (mlmap.cpp:382-386) on an explicit sensor-frame point list.
 * q_wb = (w,x,y,z), t_wb = translation of T_wb.  Returns number of points fed. */
int mlo_update_points(mlo_handle *h, const double *xyz_s, int n, const double q_wb[4], const double t_wb[3]);
/* Dense back-projection (every pixel with raw != 0, row-major, v outer) with the arithmetic of
 * mlmap.cpp:329,344-346, then update_map. */
int mlo_update_depth_dense(mlo_handle *h, const uint16_t *img, int rows, int cols, const double q_wb[4],
                           const double t_wb[3]);
/* Back-projection of an explicit pixel list (pixel = v*cols+u, in list order; raw==0 skipped). */
int mlo_update_depth_indexed(mlo_handle *h, const uint16_t *img, int rows, int cols, const int32_t *pix, int n_pix,
                             const double q_wb[4], const double t_wb[3]);
/* mlmap::project_depth verbatim (mlmap.cpp:311-349): glibc rand(), v first, <= sample_cnt points. */
int mlo_update_depth_sampled(mlo_handle *h, const uint16_t *img, int rows, int cols, const double q_wb[4],
                             const double t_wb[3]);
/* awareness stage only / local stage only (for per-stage timing and G1 fixtures) */
int mlo_awareness_points(mlo_handle *h, const double *xyz_s, int n, const double q_wb[4], const double t_wb[3]);
void mlo_local_from_awareness(mlo_handle *h);
/* back-projection alone: writes up to rows*cols points (xyz), returns count */
int mlo_project_dense(mlo_handle *h, const uint16_t *img, int rows, int cols, double *xyz_out);

/* mlmap::depth_odom_input_callback (mlmap.cpp:463-532) without ROS: 32FC1->16UC1 conversion (:480-483), pose latency
 * compensation (:485-498, Sophus SO3 log/exp so3.cpp:127-202), project_depth (rand() sampler, or dense when sampled=0),
 * update_map.  Stamps in seconds.  odom_q = (w,x,y,z).  T_wb_out (optional): q(4) + t(3) of the compensated pose. */
int mlo_callback(mlo_handle *h, const void *depth, int is_f32, int rows, int cols, double t_img, const double odom_p[3],
                 const double odom_q[4], const double odom_v[3], double t_odom, const double imu_w[3], double t_imu,
                 double camera2odom_latency, int sampled, double *T_wb_out);

/* awareness results of the last frame, in container iteration order */
size_t mlo_hit_count(mlo_handle *h);
size_t mlo_miss_count(mlo_handle *h);
void mlo_get_hits(mlo_handle *h, int32_t *rpz, float *odds);
void mlo_get_misses(mlo_handle *h, uint64_t *idx);
size_t mlo_hit_bucket_count(mlo_handle *h);
size_t mlo_out_of_range_count(mlo_handle *h); /* "point out range" branch, map_awareness.cpp:277 */
void mlo_get_T_ls(mlo_handle *h, double q[4], double t[3]);
void mlo_get_odds_table(mlo_handle *h, float *out /* 21*n_rho */);
int mlo_n_phi(mlo_handle *h);
int mlo_n_z(mlo_handle *h);

/* local map state */
size_t mlo_block_count(mlo_handle *h);
/* keys: n*3 int32; collapsed: n uint8; log_odds: n*cells float; occ / infl: n*cells char;
 * frontier_cnt: n int32.  Collapsed blocks fill element 0 only. Iteration order. */
void mlo_export_blocks(mlo_handle *h, int32_t *keys, uint8_t *collapsed, float *log_odds, char *occ, char *infl,
                       int32_t *frontier_cnt);
/* mlm_import_blocks' counterpart (same arrays as mlo_export_blocks writes; any plane may be NULL: a new block keeps allocate_ram's
 * 0 / 'u' / 'u', map_local.h:215-231, a held one that plane).  In frontier mode a block flagged collapsed keeps element 0 only, as
 * the release of map_local.cpp:221-226 leaves it.  Frontier sets are not imported. */
void mlo_import_blocks(mlo_handle *h, int n, const int32_t *keys, const float *log_odds, const char *occ, const char *infl,
                       const uint8_t *collapsed);
size_t mlo_frontier_total(mlo_handle *h);
void mlo_export_frontier(mlo_handle *h, int32_t *keys3_cell /* n*4: gx,gy,gz,cell */);

/* queries (mlmap.h:142-295, mlmap.cpp:388-407) */
void mlo_get_occupancy(mlo_handle *h, const double *pos, int n, int32_t *out);
void mlo_get_occupancy_inflate(mlo_handle *h, const double *pos, int n, float inflate, int32_t *out);
void mlo_get_inflate_occupancy(mlo_handle *h, const double *pos, int n, int32_t *out);
void mlo_get_odd(mlo_handle *h, const double *pos, int n, float *out);
void mlo_get_odd_grad(mlo_handle *h, const double *pos, int n, int max_iter, double *out3);
void mlo_set_free_in_bound(mlo_handle *h, const double bmin[3], const double bmax[3]);
/* mlmap::inflate_map (mlmap.cpp:286-309) with ct_pos = vehicle position */
void mlo_inflate_map(mlo_handle *h, const double ct_pos[3]);
/* PointCloud2 payload of pub_global_local_map (rviz_vis.cpp:296-327): float xyz of inflated 'o' cells */
size_t mlo_global_map_points(mlo_handle *h, float *xyz /* may be NULL to count */);

/* PointCloud2 payload of pub_frontier (rviz_vis.cpp:267-293): float xyz of the frontier cells' centres */
size_t mlo_frontier_points(mlo_handle *h, float *xyz /* may be NULL to count */);
/* float mlmap::getOdd(const Vec3I &glb_id, size_t subbox_id), mlmap.h:227-235 */
void mlo_get_odd_at(mlo_handle *h, const int32_t *glb_id, const int32_t *subbox_id, int n, float *out);

/* cv::Mat::convertTo(CV_16UC1, 1000) of 32FC1 pixels (mlmap.cpp:482) */
void mlo_cv_f32_to_u16(const float *in, int n, uint16_t *out);

/* The SO3 / SE3 restatements on their own (q = w,x,y,z; T = q then t), for the property tests the reference holds for
 * Sophus: 3rdPartLib/Sophus/sophus/test_so3.cpp:14-110, test_se3.cpp:10-86. */
void mlo_so3_from_quat(const double q[4], double out[4]);
void mlo_so3_exp(const double omega[3], double out[4]);
void mlo_so3_log(const double q[4], double out[3]);
void mlo_so3_mul(const double a[4], const double b[4], double out[4]);
void mlo_so3_matrix(const double q[4], double R[9]);
void mlo_se3_mul(const double a[7], const double b[7], double out[7]);
void mlo_se3_inverse(const double a[7], double out[7]);
void mlo_se3_apply(const double a[7], const double p[3], double out[3]);

#ifdef __cplusplus
}
#endif
#endif
