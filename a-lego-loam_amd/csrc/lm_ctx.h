// lm_ctx.h — device-side view of the LaserMapping state of one handle.
#ifndef ALEGO_LM_CTX_H_
#define ALEGO_LM_CTX_H_
#include "dev_common.h"
#include "lm_rows.h"

enum {
  LI_NKF = 0,      // key frames saved so far (cloud_keyposes_3d_->size())
  LI_DIRTY,        // key-frame set changed since the map was last voxel-filtered
  LI_RUN,          // mapping body runs for this scan (laserMapping.cpp:107-112)
  LI_REBUILD,      // map concat + VoxelGrid + grid rebuild this frame
  LI_FRAME,        // frame_cnt (laserMapping.cpp:111)
  LI_FLAGS,        // ALEGO_FLAG_LM_* of the last call
  LI_NCC, LI_NSC,  // corner / surf correspondences
  LI_SUM0, LI_SUM1,  // packed summaries of the two ceres::Solve calls
  LI_KF_ADDED, LI_OPTIMIZED,
  LI_KRAW_C, LI_KRAW_S, LI_KDS_C, LI_KDS_S,
  LI_NIN_C, LI_NIN_S, LI_NIN_O,          // staged inputs (/corner_last, /surf_last, /outlier)
  LI_NCUR_C, LI_NCUR_S, LI_NCUR_O,       // laser_corner_ds_, laser_surf_ds_, laser_outlier_ds_
  LI_NTOTAL, LI_NTOTAL_DS,               // laser_surf_total_, laser_surf_total_ds_
  LI_NREBUILD,     // map rebuilds so far (bench: expected work of the map VoxelGrid kernels)
  LI_OVERFLOW,     // a capacity was exceeded (1: clouds truncated, 8: a window beyond the voxel-key range) or an internal check failed (2, 4): reported as an error by the host
  LI_REC_CNT,      // recent_*_keyframes_.size() (laserMapping.cpp:208)
  LI_LATEST,       // latest_frame_id_ (laserMapping.cpp:226), -1 until the deque has been full once
  LI_NU_C, LI_NU_S,      // occupied voxels of the corner / surf local map (size of the sorted voxel-key lists U)
  LI_UVALID,       // U / Ucnt describe the window in rec_prev (cleared by everything that changes key frames behind their back)
  LI_PREV_CNT,     // entries of rec_prev
  LI_KF_PENDING,   // a key frame was written to kf_tmp_* and still has to be sorted into ring entry LI_KF_PEND_RING
  LI_KF_PEND_RING,
  LI_TMPN_C, LI_TMPN_S,  // points in kf_tmp_c / kf_tmp_s
  LI_REBUILD_FB,   // LI_REBUILD on the concat + radix VoxelGrid path (ALEGO_MAP_MERGE=0)
  LI_MAP_PASS,     // bit m: map m took PCL's "leaf size too small" path in map_update (output = input), map_accum skips it;
                   // bit 2 + m: map m was refused because its window does not fit the voxel key (LI_OVERFLOW 8, no list and no map)
  LI_SORT_N,       // (2 entries) point counts written by the key-frame sort jobs
  LI_SORT_N1,
  LI_TM_FAST,      // mapping frames whose laser_surf_total_ds_ lm_total_merge built by merging (kernels_lm.hip) ...
  LI_TM_LIST,      // ... and frames it refused, whose round-2 job went on the VoxelGrid work list (tests: which path a scene took)
  LI_COUNT = 48
};
enum {
  LD_PARAMS = 0,     // params_[6] (absolute map pose)
  LD_T_M2O = 6, LD_Q_M2O = 9,    // map -> odom
  LD_T_O2L = 13, LD_Q_O2L = 16,  // odom -> laser (last /odom/lidar)
  LD_T_M2L = 20, LD_Q_M2L = 23,  // map -> laser
  LD_PARAMS_IT = 27,             // params_ after each outer iteration [2][6]
  LD_COSTS = 39,                 // initial/final cost of both solves
  LD_LOC_P = 44,                 // localisation (kernels_loc.hip): the f32 position the last mapping frame selected its window with, x y z (44..46)
  LD_COUNT = 48
};

struct alego_graph_edge;   // include/alego_mi355x.h
struct alego_regcov;
struct alego_remap;

struct MapWork {     // work list of map_accum, written by map_update (kernels_map.hip)
  int* items;      // [cap] packed (slot - slot0) << 12 | m << 11 | chunk   (chunk < 2048)
  int* count;      // [2]: items, ticket
  int cap;
};
struct LtLists { int *list_small, *list_big, *cnt, *cnt_next; int small_max; };   // work lists of the round-2 VoxelGrid context (voxel.h): cnt this launch's two list sizes (zero on entry), cnt_next the set it zeroes for the next launch
struct GridGeom { int ox, oy, oz; float inv; int gx, gy, gz, ncell; };   // cell of x: floorf(x * inv) - ox (lm_grid_build)


// f32 4x4 of transformPointCloud (laserMapping.h:166-173): AngleAxisf(yaw,Z)*AngleAxisf(pitch,Y)*AngleAxisf(roll,X).
// sin/cos of the half angles are glibc's sinf / cosf (dev_common.h), as Eigen's Quaternionf(AngleAxisf) calls them.
DEV_INLINE void keypose_matrix(const float* kp, float m[3][4]) {
  const float hz = 0.5f * kp[5], hy = 0.5f * kp[4], hx = 0.5f * kp[3];
  const float qz[4] = {d_cosf(hz), 0.f, 0.f, d_sinf(hz)};
  const float qy[4] = {d_cosf(hy), 0.f, d_sinf(hy), 0.f};
  const float qx[4] = {d_cosf(hx), d_sinf(hx), 0.f, 0.f};
  float t[4], q[4];
  t[0] = qz[0] * qy[0] - qz[1] * qy[1] - qz[2] * qy[2] - qz[3] * qy[3];
  t[1] = qz[0] * qy[1] + qz[1] * qy[0] + qz[2] * qy[3] - qz[3] * qy[2];
  t[2] = qz[0] * qy[2] + qz[2] * qy[0] + qz[3] * qy[1] - qz[1] * qy[3];
  t[3] = qz[0] * qy[3] + qz[3] * qy[0] + qz[1] * qy[2] - qz[2] * qy[1];
  q[0] = t[0] * qx[0] - t[1] * qx[1] - t[2] * qx[2] - t[3] * qx[3];
  q[1] = t[0] * qx[1] + t[1] * qx[0] + t[2] * qx[3] - t[3] * qx[2];
  q[2] = t[0] * qx[2] + t[2] * qx[0] + t[3] * qx[1] - t[1] * qx[3];
  q[3] = t[0] * qx[3] + t[3] * qx[0] + t[1] * qx[2] - t[2] * qx[1];
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  m[0][0] = 1 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy; m[0][3] = kp[0];
  m[1][0] = txy + twz; m[1][1] = 1 - (txx + tzz); m[1][2] = tyz - twx; m[1][3] = kp[1];
  m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1 - (txx + tyy); m[2][3] = kp[2];
}

DEV_INLINE float4 kf_transform(const float m[3][4], const float4& p) {   // laserMapping.h:175 (pcl::transformPointCloud, f32)
  float4 o;
  o.x = m[0][0] * p.x + m[0][1] * p.y + m[0][2] * p.z + m[0][3];
  o.y = m[1][0] * p.x + m[1][1] * p.y + m[1][2] * p.z + m[1][3];
  o.z = m[2][0] * p.x + m[2][1] * p.y + m[2][2] * p.z + m[2][3];
  o.w = p.w;
  return o;
}

struct LmCtx {
  int K;                         // recent_keyframe_num
  // Where the key frames of a slot live: kf_row / kf_run_at (kf_store.h) find frame f of slot s in kfs_* / kf_raw_* / kf_cnt / kf_pose from these two.  SLAM: the slot's own
  // ring, fr_stride = fr_mod = KR.  Localisation (alego_loc_enable): those pointers name ONE frozen map store shared by every slot, fr_stride = 0 and fr_mod = its frame capacity.
  int fr_stride, fr_mod;
  int loc_on, loc_n;             // localisation mode; frames of the map store
  float loc_r2;                  // (float)(radius * radius) of loc_select
  int KR;                        // ring entries per slot = K + 1: frame f lives in entry f % KR, so the frame a full window pops
                                 // (f - K) is still intact when the frame that pushes it out (f) has been stored
  int kf_cap_c, kf_cap_s, kf_cap_o;
  int in_cap_c, in_cap_s, in_cap_o;
  int map_cap_c, map_cap_s;      // K*kf_cap_c, K*(kf_cap_s+kf_cap_o)
  int total_cap;                 // kf_cap_s + kf_cap_o
  int gcap;                      // grid cells capacity per map
  int qcap;                      // residual rows capacity: kf_cap_c + total_cap
  int solve_row_bytes;           // LDS lm_solve keeps its accepted rows in (ALEGO_LM_ROW_LDS overrides; rows beyond it are read from crows)
  int* li;                       // [slot][LI_COUNT]
  double* ld;                    // [slot][LD_COUNT]
  // staged inputs
  float4 *in_corner, *in_surf, *in_outl;          // [slot][in_cap_*]
  double* stage_odom;                             // [slot][2][8] /odom/lidar of a scan (t 3, q 4, valid) handed over by lm_stage when LaserMapping runs on a
                                                  // HIP stream of its own behind the front end (double-buffered by scan parity)
  // key-frame ring (clouds already transformed into the map frame, laserMapping.cpp:216-218) and SORTED by voxel key of the
  // map's leaf size (stable: input order inside a voxel): corner, and surf followed by outlier (:240-242) as one run
  float4 *kfs_c, *kfs_s;                          // [slot][KR][kf_cap_c] / [slot][KR][total_cap]
  int* kfs_n;                                     // [slot][2][KR] points per run (kf_run_at)
  float* kfs_box;                                 // [slot][2][KR][8] min xyz (0..2) / max xyz (4..6) of the run
  float4 *kf_tmp_c, *kf_tmp_s;                    // [slot][kf_cap_c] / [slot][total_cap] transformed clouds of the key frame waiting to be sorted
  // sorted list of the occupied voxels of each local map (persistent, updated incrementally when the window changes)
  unsigned long long *U_c, *U_s;                  // [slot][map_cap_*]
  int *Ucnt_c, *Ucnt_s;                           // [slot][map_cap_*] points per voxel
  int* rec_prev;                                  // [slot][K] window the lists describe (ring frame ids, front first)
  float4* newkeys;                                // [slot][2][total_cap] scratch of map_update: (key lo, key hi, lower bound, count) of the voxels a run adds
  // ---- one registration sharded over the ranks of a communicator (alego_dist_*; kernels lm_shard_*) ----
  int shard_rank, shard_world;                    // world 0: not sharded
  double* shard_part;                             // [slot][32] this rank's partial sums of an evaluation: 21 J^T J, 6 J^T r, cost, corner / surf rows; all-reduced in place
  void* shard_state;                              // [slot] LmState of the solve in flight (solve_rows.h)
  int* shard_ctl;                                 // [slot][8]: 0 local rows, 1 action of the last step, 2 solve finished, 3 outer iteration, 4 guard failed
  unsigned* map_bbox;                             // [slot][2][8] bounding box of the window's points in the VoxelGrid kernels' encoding (vgrid.h; merge path)
  // the same key frames as saveKeyFramesAndFactor stores them (sensor frame, :553-555): host read-back + pose correction
  float4 *kf_raw_c, *kf_raw_s, *kf_raw_o;         // [slot][KR][kf_cap_*]
  int* rec;                                       // [slot][K] frame ids held by recent_*_keyframes_, front first
  int* kf_cnt;                                    // [slot][KR][4]
  float* kf_pose;                                 // [slot][KR][8]  x y z roll pitch yaw (PointXYZIRPYT f32)
  // local map
  float4 *map_corner_raw, *map_surf_raw;          // [slot][map_cap_*]
  float4 *map_corner_ds, *map_surf_ds;
  // current scan
  float4 *cur_corner_ds, *cur_surf_ds, *cur_outl_ds, *cur_total, *cur_total_ds;
  // uniform grid over the down-sampled maps (index 0 corner, 1 surf)
  GridGeom* grid;                                 // [slot][2]
  int *cell_start, *cell_cur;                     // [slot][2][gcap+1]
  float4* cell_pts;                               // [slot][2][map_cap_s] map points in cell order (w = index in the ds map)
  const unsigned* vox_bbox;                       // VoxCtx::bbox of round 1 of this stream group (the map VoxelGrid context: jobs (slot-vox_slot0)*2 + {0,1})
  int vox_slot0;                                  // first slot of the stream group
  int* knn;                                       // [slot][qcap][LM_KNN_W] neighbour indices of every query, at the rows of `blocks` (lm_knn -> lm_fit)
  // residual blocks
  double* blocks;                                 // [slot][qcap][LMB_W]: the block record of every query (lm_rows.h)
  double* crows;                                  // [slot][qcap][LMS_W]: accepted rows that do not fit lm_solve's LDS (all rows on the sharded path), as streamed records (lm_rows.h)
  // key-frame archive (alego_map_enable; arc_frames_cap == 0: off, nothing is launched): EVERY key frame of a slot as the ring stores it
  // (sensor frame, kf_raw_* / kf_cnt) + its f32 key pose, appended by map_archive behind lm_store_kf; the stored frames are always a prefix
  int arc_frames_cap, arc_points_cap;             // per slot
  float4* arc_pts;                                // [slot][arc_points_cap] corner | surf | outlier of each frame, frames back to back
  int* arc_tab;                                   // [slot][arc_frames_cap][4] point offset, n corner, n surf, n outlier
  float* arc_pose;                                // [slot][arc_frames_cap][8] x y z roll pitch yaw
  int* arc_stat;                                  // [slot][4] frames stored, frames dropped, points stored, -
  double* arc_stamp;                              // [slot][arc_frames_cap] stamp of each frame (detectLoopClosure's key-pose time, :782)
  int* arc_stamped;                               // [slot] 1: DevCtx::scan_stamp holds the slot's scan stamps (alego_scan_process / alego_lo_process);
                                                  // 0: the stamp is (LI_FRAME - 1) * scan_period
  // key-pose graph next to the archive (alego_graph_enable; pg_loops_cap == 0: off, nothing is launched or allocated): the prior and
  // the odometry chain recorded by map_archive as frames are appended, the loop edges the host added, the last optimise's estimate
  int pg_loops_cap;                               // loop edges per slot
  double pg_odom_var[6];                          // variances of the prior and of every odometry edge (laserMapping.cpp:68-70)
  alego_graph_edge* pg_chain;                     // [slot][arc_frames_cap] edge i: the prior (i = 0, from = -1) or i - 1 -> i
  alego_graph_edge* pg_loops;                     // [slot][pg_loops_cap]
  float* pg_corr;                                 // [slot][16] ICP correction of the last loop edge added (correctPoses :579-580)
  int* pg_stat;                                   // [slot][4] loop edges stored, loop_closed_ (a loop edge was added since the last apply), poses of the estimate, -
  double* pg_est;                                 // [slot][arc_frames_cap][12] Pose3 estimate of the slot's last optimise, row-major [R | t]
  // registration covariance (alego_regcov_enable; rc_rec == nullptr: off, nothing is launched or allocated): one record per slot, written by
  // lm_regcov between the solver and lm_finish
  alego_regcov* rc_rec;                           // [slot]
  const double* rc_opt;                           // [RC_OPT_W] the resolved options (reg_cov_math.h)
  int rc_graph;                                   // 1: map_archive writes a fresh record's variances into the odometry edge it records
  // solution remapping (alego_remap_enable; rm_rec == nullptr: off, nothing is allocated and lm_solve runs): one record per slot, written by
  // lm_solve_remap behind the first evaluation of a mapping frame
  alego_remap* rm_rec;                            // [slot]
  double rm_eig_min;                              // the resolved option (remap_math.h)
};

// a slot's rows (lm_rows.h: a corner query q has row q, a surf query q row kf_cap_c + q)
DEV_INLINE double* lm_blocks_of(const LmCtx& L, int slot) { return L.blocks + (size_t)slot * L.qcap * LMB_W; }
DEV_INLINE double* lm_crows_of(const LmCtx& L, int slot) { return L.crows + (size_t)slot * L.qcap * LMS_W; }
DEV_INLINE int* lm_knn_of(const LmCtx& L, int slot, int kind, int q) { return L.knn + ((size_t)slot * L.qcap + lm_row_of(kind, q, L.kf_cap_c)) * LM_KNN_W; }

// The registration guard (:350) of lm_knn, lm_fit and both solver paths ("no map yet": see kernels_lm.hip), and what the solver path leaves of a
// skipped registration
DEV_INLINE bool lm_reg_skipped(const int* li, const alego_params& P) {
  return lm_guard_fails(li[LI_NCUR_C], li[LI_NTOTAL], li[LI_KDS_C], (li[LI_NKF] | li[LI_REC_CNT]) == 0, P.lm_min_corner, P.lm_min_surf, P.lm_min_map_corner);
}
DEV_INLINE void lm_store_skipped(int* li) { li[LI_FLAGS] |= 16; li[LI_NCC] = 0; li[LI_NSC] = 0; li[LI_SUM0] = 0; li[LI_SUM1] = 0; }
// one thread, when outer iteration `outer` has ended: params_ and the summaries of its ceres::Solve ...
DEV_INLINE void lm_store_outer(int* li, double* ld, int outer, const LmState& S) {
#pragma unroll
  for (int k = 0; k < 6; ++k) ld[LD_PARAMS + k] = S.x[k];
  if (outer < 2) {
    for (int k = 0; k < 6; ++k) ld[LD_PARAMS_IT + outer * 6 + k] = S.x[k];
    ld[LD_COSTS + outer * 2] = S.initial_cost; ld[LD_COSTS + outer * 2 + 1] = S.x_cost;
    li[LI_SUM0 + outer] = S.iter | (S.successful << 8) | (S.termination << 16);
  }
}
// ... and of one without rows: ceres::Solve on an empty problem is a no-op
DEV_INLINE void lm_store_outer_empty(int* li, double* ld, int outer) {
  if (outer < 2) {
    li[LI_SUM0 + outer] = 4 << 16;
    for (int k = 0; k < 6; ++k) ld[LD_PARAMS_IT + outer * 6 + k] = ld[LD_PARAMS + k];
  }
}

// host entry points of LaserMapping's kernels (kernels_lm.hip, then kernels_map.hip and kernels_loc.hip), called by lm_host.hip; lm_configure: by alego_create
size_t lm_solve_row_bytes_max(), lm_solve_row_bytes_default();
int lm_configure();
void launch_lm_prepare(const DevCtx& d, const LmCtx& L, int stage, int run_hint, int par, hipStream_t st);
void launch_lm_stage(const DevCtx& d, const LmCtx& L, int run_hint, int par, hipStream_t st);
void launch_lm_concat(const DevCtx& d, const LmCtx& L, hipStream_t st);
void launch_lm_total(const DevCtx& d, const LmCtx& L, hipStream_t st);
void launch_lm_total_merge(const DevCtx& d, const LmCtx& L, const LtLists& W, hipStream_t st);
void launch_lm_grid(const DevCtx& d, const LmCtx& L, hipStream_t st);
void launch_lm_solve(const DevCtx& d, const LmCtx& L, bool remap, hipStream_t st);   // the solver kernel alone (launch_lm_register's, and alego_debug_remap_solve's on a one-slot view)
int launch_lm_register(const DevCtx& d, const LmCtx& L, hipStream_t st, int (*allreduce)(void*, double*, size_t, hipStream_t), void* ar_ctx);
void launch_lm_retransform(const DevCtx& d, const LmCtx& L, int ring, hipStream_t st);
void launch_lm_apply_correction(const DevCtx& d, const LmCtx& L, int slot, const double* rc_dev, hipStream_t st);
// lm_regcov's evaluation and 6x6 part on caller-supplied rows: blocks [n_edge + n_plane][8] (edges first), their query points, p[6], options, one record
void launch_lm_regcov_debug(const double* blocks, const float4* qc, int n_edge, const float4* qs, int n_plane, const double* params, double huber, const double* opt,
                            alego_regcov* rec, hipStream_t st);
// host twins: the record from 28 scalars and resolved options (reg_cov_math.h); the 28 scalars from rows (a, b, p | n, d, p), edges then planes, in row order
void regcov_host(const double* acc28, const double* params6, int n_edge, int n_plane, const double* opt, alego_regcov* out);
void regcov_normal_host(const double* params6, const double* edge_rows9, int n_edge, const double* plane_rows7, int n_plane, double huber, double* acc28);
// host twins of lm_solve_remap's 6x6 part and of one lm_step (remap_math.h, solve_rows.h)
void remap_host(const double* acc28, const double* params6, int n_edge, int n_plane, double eig_min, alego_remap* out);
int remap_step_host(const double* H21, const double* g6, const double* scale6, double radius, const double* proj36, double* step6, double* mcc);
void launch_map_update(const DevCtx& d, const LmCtx& L, const MapWork& W, hipStream_t st);
void launch_map_accum(const DevCtx& d, const LmCtx& L, const MapWork& W, hipStream_t st);
void launch_loc_select(const DevCtx& d, const LmCtx& L, hipStream_t st);

#endif
