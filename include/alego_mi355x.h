/*
 * alego_mi355x.h — C ABI of the MI355X-native A-LeGO-LOAM hot path.
 *
 * The reference has no FFI: its boundary is three ROS nodelets exchanging
 * messages (nodelet_plugins.xml:1-10).  Each entry point below replaces the
 * numeric body of one nodelet callback and takes / returns exactly the payload
 * of the ROS messages that callback consumes / publishes, as plain pointers and
 * sizes.  A thin adapter keeps plugin names, topics and frames.
 *
 *   alego_ip_process   <- ImageProjection::pcCB            src/imageProjection.cpp:49-208
 *   alego_lo_process   <- LaserOdometry::mainLoop body     src/laserOdometry.cpp:111-553
 *   alego_lm_process   <- LaserMapping::mainLoop body +    src/laserMapping.cpp:112-123,
 *                         laserOdomHandler                 154-166
 *   alego_scan_process <- the three chained in one process (launch/test.launch: one
 *                         nodelet manager), intermediates stay in HBM
 *   alego_batch_*      <- bag replay at unbounded rate (README.md:33-37) over many
 *                         independent streams, inputs resident in HBM, no per-scan
 *                         host synchronisation
 *
 * All functions return 0 on success, >0 for the reference's "skip" conditions
 * (surfaced as flags, see ALEGO_FLAG_*), <0 for hard errors (ALEGO_ERR_*); nothing
 * throws across the boundary.  A handle is single-threaded (one caller at a time;
 * it owns its HIP streams); different handles are independent.  There is no CPU fallback:
 * alego_create fails with ALEGO_ERR_NO_DEVICE when no gfx950 device is visible.
 */
#ifndef ALEGO_MI355X_H_
#define ALEGO_MI355X_H_

#include <stdint.h>

#include "alego_params.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct alego_handle alego_handle;

enum {
  ALEGO_OK = 0,
  ALEGO_ERR_NO_DEVICE = -1, /* no HIP device / not gfx950 */
  ALEGO_ERR_HIP = -2,       /* a HIP call failed, see alego_last_error */
  ALEGO_ERR_CAPACITY = -3,  /* caller buffer too small */
  ALEGO_ERR_ARG = -4
};
/* bit flags returned by the *_process calls (reference guards, not errors) */
enum {
  ALEGO_FLAG_LO_INIT = 1,        /* first scan: features stored, no odometry   laserOdometry.cpp:316-324 */
  ALEGO_FLAG_FEW_SURF = 2,       /* < lo_min_corr surf correspondences         laserOdometry.cpp:422-425 */
  ALEGO_FLAG_FEW_CORNER = 4,     /* < lo_min_corr corner correspondences       laserOdometry.cpp:496-499 */
  ALEGO_FLAG_LM_SKIPPED = 8,     /* odd mapping frame                          laserMapping.cpp:112 */
  ALEGO_FLAG_LM_FEW_FEATURES = 16, /* registration guard                       laserMapping.cpp:350-354 */
  ALEGO_FLAG_LM_KEYFRAME = 32    /* a key frame was saved                      laserMapping.cpp:491-559 */
};

/* ---- messages ------------------------------------------------------------ */
/* /lslidar_point_cloud (sensor_msgs/PointCloud2 as PointXYZI) */
typedef struct alego_scan_in {
  const alego_point* pts;
  int32_t n;
  double stamp;
} alego_scan_in;

/* /segmented_cloud + /seg_info (msg/cloud_info.msg:1-12) + /outlier.
 * Caller owns every buffer; capacities are in elements; worst case is
 * n_scan*horizon_scan for seg/ground/col/range/outlier/label_image. */
typedef struct alego_seg_out {
  alego_point* seg;      int32_t seg_cap;  int32_t m;          /* segmented_cloud */
  uint8_t* ground;       /* segmentedCloudGroundFlag[m] */
  int32_t* col;          /* segmentedCloudColInd[m]     */
  float* range;          /* segmentedCloudRange[m]      */
  int32_t* ring_start;   /* startRingIndex[n_scan]      */
  int32_t* ring_end;     /* endRingIndex[n_scan]        */
  float orientation[3];  /* startOrientation, endOrientation, orientationDiff */
  alego_point* outlier;  int32_t outlier_cap;  int32_t n_outlier;
  int32_t* label_image;  /* optional (may be NULL): label_mat_ [n_scan][horizon_scan] */
  double stamp;          /* header stamp of /segmented_cloud + /seg_info = the input scan's (t1 of laserOdometry.cpp:111; read by the de-skew) */
} alego_seg_out;

/* /corner, /corner_less, /surf, /surf_less (laserOdometry.cpp:299-314); the
 * less_* clouds are also /corner_last and /surf_last (:531-546). */
typedef struct alego_feat_out {
  alego_point* sharp;       int32_t sharp_cap;       int32_t n_sharp;
  alego_point* less_sharp;  int32_t less_sharp_cap;  int32_t n_less_sharp;
  alego_point* flat;        int32_t flat_cap;        int32_t n_flat;
  alego_point* less_flat;   int32_t less_flat_cap;   int32_t n_less_flat;
  int32_t* point_label;     /* optional (may be NULL): cloud_label_[m] */
} alego_feat_out;

/* nav_msgs/Odometry pose (/odom/lidar, /odom_aft_mapped) + the 6-vector the solver works on */
typedef struct alego_pose {
  double t[3];
  double q[4];      /* w, x, y, z */
  double params[6]; /* LO: last relative transform; LM: absolute map pose (x,y,z,roll,pitch,yaw) */
  int32_t valid;
} alego_pose;

/* ---- lifecycle ------------------------------------------------------------ */
/* n_slots independent streams share one handle (batch path); the single-scan
 * entry points use slot 0.  ring_len = scans kept resident per slot for the
 * batch path (0 -> 1). */
int alego_create(const alego_params* params, int device, int n_slots, int ring_len, alego_handle** out);
void alego_destroy(alego_handle* h);
const char* alego_last_error(const alego_handle* h);
int alego_device_count(void);
/* size of alego_params this library was built with (binding sanity check) */
int alego_params_sizeof(void);
/* A handle is single-threaded: one caller at a time.  A host that drives ONE handle from several threads — the three nodelets of
 * launch/test.launch:6-10 share a process, the reference serialises them with per-node mutexes (laserOdometry.cpp:93,548;
 * laserMapping.cpp:114,729,769) — brackets every call (and every group of calls that must see a consistent handle) with this
 * recursive lock, which lives in the handle so that all users of the handle share it. */
int alego_handle_lock(alego_handle* h);
int alego_handle_unlock(alego_handle* h);

/* ---- nodelet-equivalent single-scan entry points (host buffers, slot 0) --- */
int alego_ip_process(alego_handle* h, const alego_scan_in* in, alego_seg_out* out);
/* `in` is the IP output as received on /segmented_cloud + /seg_info; `odom` is /odom/lidar */
int alego_lo_process(alego_handle* h, const alego_seg_out* in, alego_feat_out* feat, alego_pose* odom);
/* inputs: /corner_last, /surf_last, /outlier, /odom/lidar; output: /odom_aft_mapped and params_ */
int alego_lm_process(alego_handle* h, const alego_point* corner_last, int32_t n_corner,
                     const alego_point* surf_last, int32_t n_surf, const alego_point* outlier,
                     int32_t n_outlier, const alego_pose* odom, alego_pose* map_pose);
/* IP -> LO -> LM for one scan with intermediates kept on the device.  stages: bit0 IP,
 * bit1 LO, bit2 LM.  seg/feat may be NULL (then nothing but the poses is copied back). */
int alego_scan_process(alego_handle* h, int slot, const alego_scan_in* in, int stages,
                       alego_seg_out* seg, alego_feat_out* feat, alego_pose* odom, alego_pose* map_pose);

/* ---- device-resident batch path ------------------------------------------ */
/* copy one scan into ring position `ring_pos` of `slot` (host -> HBM, outside the timed region) */
int alego_batch_load(alego_handle* h, int slot, int ring_pos, const alego_point* pts, int32_t n);
/* advance every slot by n_scans scans (ring positions first_pos, first_pos+1, ... mod ring_len),
 * all kernels enqueued on the handle's streams; returns without synchronising when sync == 0.  With sync == 0 LaserMapping of the
 * last scans may still be in flight on the stream groups' second ("back") HIP streams when the call returns: every entry point that
 * touches LaserOdometry / LaserMapping state waits for it first (per-slot calls for their own group, alego_lo_process /
 * alego_lm_process / alego_dist_init / alego_dist_shutdown for all groups; alego_stream_run orders its streams behind it on the device);
 * alego_batch_load, which only writes the input ring, does not.  A handle of G stream groups drives G HIP streams, or 2 G where every
 * group has a back stream; the HIP runtime maps them onto the process's hardware queues, and streams that share a queue serialise.
 * The number of queues is the host's setting (GPU_MAX_HW_QUEUES; the HIP runtime's default is 4): the library reads it, never sets
 * it, and fits its streams to it (alego_stream_plan). */
int alego_batch_run(alego_handle* h, int first_pos, int n_scans, int stages, int sync);
int alego_synchronize(alego_handle* h);
/* OR into `stages` of alego_batch_run: replay the resident ring back and forth (0..R-1,R-2..0,1..)
 * instead of wrapping, so that consecutive scans of a stream are always trajectory neighbours */
#define ALEGO_REPLAY_PINGPONG 0x100
/* Bag store: n_bags recorded streams of bag_len scans each, resident in HBM once and SHARED by the slots (a 560-scan lap of a
 * 16x1800 sensor is 258 MB; a private copy per slot would not fit).  alego_replay_assign makes `slot` replay `bag` from
 * scan `start_scan` on, cyclically; alego_batch_run with ALEGO_REPLAY_BAG in `stages` then advances every slot by n_scans
 * scans of its bag: first_pos is the step index (slot s processes scan (start_scan + first_pos + i) mod bag_len at step i). */
#define ALEGO_REPLAY_BAG 0x200
int alego_replay_create(alego_handle* h, int n_bags, int bag_len);
int alego_replay_load(alego_handle* h, int bag, int scan, const alego_point* pts, int32_t n);
int alego_replay_assign(alego_handle* h, int slot, int bag, int start_scan);
/* ONE stream replayed from the bag store as fast as the device allows (BASELINE config 3 as written: a single bag).  Slot 0 carries
 * the stream's state; the other slots of the handle are look-ahead lanes in two sets of W = (n_slots - 1) / 2: ImageProjection and feature
 * extraction have no state across scans, so they run for W scans ahead in one launch per kernel (one scan per lane), while LaserOdometry
 * (sequential by nature: params_, the previous scan's features) and LaserMapping (the key-frame map) follow scan by scan on two
 * further HIP streams, each started by an event of its producer — the three-nodelet pipeline of launch/test.launch on the device.
 * Results are bit-identical to alego_batch_run on a one-slot handle.  The handle needs n_slots >= 3 (odd) and a bag store;
 * `first_step` / `n_scans` as in alego_batch_run with ALEGO_REPLAY_BAG (scan (start_scan + first_step + i) mod bag_len at step i). */
int alego_stream_setup(alego_handle* h, int bag, int start_scan);
int alego_stream_run(alego_handle* h, int first_step, int n_scans, int stages, int sync);
/* poses of the last processed scan of `slot` */
int alego_batch_get_pose(alego_handle* h, int slot, alego_pose* odom, alego_pose* map_pose);
/* Per-scan pose log: what a bag replay publishes on /odom/lidar (laserOdometry.cpp:513-529) and /odom_aft_mapped
 * (laserMapping.cpp:167-181) for every scan, kept on the device so that alego_batch_run needs no host synchronisation per scan
 * (the bench-path export with a poses_out argument that SURVEY.md 8b proposes).  After alego_trajectory_enable(h, capacity) every scan a slot processes through
 * alego_batch_run / alego_scan_process appends 14 doubles: odometry t(3) q(4: w x y z), map pose t(3) q(4).  alego_trajectory_get
 * copies entries [first, first + n) of `slot` and returns the number of scans logged so far (entries beyond the capacity are
 * dropped, the count keeps running). */
int alego_trajectory_enable(alego_handle* h, int32_t capacity_scans);
int alego_trajectory_get(alego_handle* h, int slot, int32_t first, int32_t n, double* out14);
/* per-scan device counters of the last processed scan of `slot`:
 * out[0..] = P (valid input points), M, n_outlier, n_sharp, n_less_sharp, n_flat, n_less_flat,
 *            n_surf_corr, n_corner_corr, lm: Kraw_corner, Kraw_surf, Kds_corner, Kds_surf, Lc, Ls,
 *            map rebuilds so far */
int alego_batch_get_counts(alego_handle* h, int slot, int32_t* out, int cap);
/* the HIP stream (hipStream_t) the handle enqueues slot 0 on, for event timing by the caller */
void* alego_stream(alego_handle* h);
/* The slots of a handle are split into contiguous groups, each enqueued on its own HIP stream so that the kernels of
 * different groups overlap (slots never interact).  Returns the number of groups; *slots_per_group (may be NULL) =
 * slots one kernel launch covers.  Default: one group per 64 slots, at most 4 and no more than the hardware queues of the process
 * serve (alego_stream_plan); ALEGO_STREAM_GROUPS=<n> overrides. */
int alego_stream_groups(const alego_handle* h, int* slots_per_group);
/* The handle's stream plan: out[0] = stream groups, out[1] = slots per group, out[2] = 1 if every group has a back stream (LaserMapping
 * of scan k overlaps the front end of scans k + 1, k + 2 in alego_batch_run), out[3] = Q, the hardware queues the plan was fitted to:
 * ALEGO_HW_QUEUES if set, else GPU_MAX_HW_QUEUES, else 4.  What the caller does not ask for (ALEGO_STREAM_GROUPS, ALEGO_LM_ASYNC) is
 * chosen so that groups x (1 + back stream) <= Q; from Q = 8 on that is 4 groups with a back stream each.  Both variables set are taken
 * as they are at any Q.  alego_stream_run uses min(3, Q) streams.  Results never depend on the plan. */
int alego_stream_plan(const alego_handle* h, int out[4]);

/* ---- per-kernel timing (bench.py's roofline leg) --------------------------- */
/* When enabled every kernel launch of this handle is bracketed by hipEventRecord on the handle's
 * stream.  Off by default; the benchmark's timed region runs with it off. */
int alego_profile_enable(alego_handle* h, int on);
/* names: ';'-separated kernel names; total_ms / launches per kernel.  Returns the kernel count. */
int alego_profile_report(alego_handle* h, char* names, int names_cap, double* total_ms, int* launches, int cap);

/* ---- motion de-skew (LaserOdometry::adjustDistortion, laserOdometry.cpp:557-726; alego_params.deskew_mode = 1) --------------
 * sensor_msgs/Imu as LaserOdometry::imuHandler (:761-802) receives it.  The handler's ring of 200 dead-reckoned samples lives on
 * the device; with deskew_mode = 1 every scan's segmented cloud is de-skewed against it before feature extraction (the call the
 * reference has commented out at :115), by alego_lo_process / alego_scan_process (the stamps come from alego_seg_out.stamp /
 * alego_scan_in.stamp).  Stamps must not decrease. */
typedef struct alego_imu {
  double stamp;
  double orientation[4];          /* w, x, y, z */
  double linear_acceleration[3];
  double angular_velocity[3];     /* carried by the message, unused by the reference (:787-789) */
} alego_imu;
int alego_lo_push_imu(alego_handle* h, int slot, const alego_imu* samples, int32_t n);
/* /undistorted (src/laserOdometry.cpp:56,718-725; src/LO.cpp:127,797-804): the de-skewed segmented cloud of `slot`'s last scan, as adjustDistortion
 * publishes it when somebody subscribes.  Returns the number of points, ALEGO_ERR_ARG when deskew_mode = 0 (the reference then never publishes on the
 * topic either: the call is commented out at laserOdometry.cpp:115), ALEGO_ERR_CAPACITY when `cap` is too small. */
int alego_lo_get_undistorted(alego_handle* h, int slot, alego_point* out, int32_t cap);
/* The STANDALONE LaserOdometry node's frame convention (src/LO.cpp:588-608): /odom/lidar is published as /odom -> /base_link with
 * tf_o2b = tf_o2l * tf_b2l^-1 (tf_b2l: base_link -> laser mount, row-major 4 x 4; identity at LO.cpp:121), its quaternion taken from the rotation
 * block; the nodelet (src/laserOdometry.cpp:513-529) publishes /odom -> /laser unchanged.  Host arithmetic: `o2l` is what alego_lo_process returned,
 * `o2b` gets t and q (params / valid copied).  ALEGO_ERR_ARG for a singular tf_b2l. */
int alego_pose_o2b(const alego_pose* o2l, const double* tf_b2l, alego_pose* o2b);

/* ---- state access for parity tests (teacher forcing) ---------------------- */
int alego_set_lo_params(alego_handle* h, int slot, const double* p6);
int alego_set_lm_params(alego_handle* h, int slot, const double* p6);
/* copy a named device intermediate of `slot` to host; *count = number of scalars written.
 * dtype: 0 f32, 1 f64, 2 i32, 3 u8.  Names mirror oracle_get().  Of the fused feature extraction's candidate kernel (fe_cand) for the slot's
 * last scan, as i32: "fe_cand_span" = {sectors of a ring per wavefront (0: all; ALEGO_FE_SPAN=1: one), sector_cap}, "fe_cand_counts" =
 * [ring][sector]{sharp, flat candidates}, "fe_cand_lists" = [ring][sector][sector_cap]{key, pay}: the sharp candidates from the front of a
 * sector's list, the flat ones from its back (fe_pickc clears the keys of entries it picks from memory). */
int alego_debug_get(alego_handle* h, int slot, const char* name, void* out, int cap_bytes,
                    int* count, int* dtype);
/* the device pcl::VoxelGrid replacement on a host cloud (the LDS-resident radix sort for <= 8192 points, the HBM-scratch
 * radix sort above), for direct parity tests against the oracle; returns the output count */
int alego_debug_voxel(alego_handle* h, const alego_point* pts, int n, float leaf, alego_point* out, int cap);
/* device atan2f / hypotf used by the projection kernel, for the libm-equivalence test */
int alego_debug_atan2f(alego_handle* h, const float* y, const float* x, float* out, int n);
/* libstdc++ std::sort(idx, idx + n, [](a, b) { return keys[a] < keys[b]; }) on idx = 0..n-1 (n <= 4096) as the device reproduces
 * it for alego_params.sort_mode = 2 (laserOdometry.cpp:185): order[k] = the element at sorted position k.  depth_limit < 0 = std::sort's
 * own 2 floor(log2 n); >= 0 overrides __introsort_loop's depth limit (0 = heap sort at once) so that tests reach that branch */
int alego_debug_std_sort(alego_handle* h, const uint32_t* keys, int n, int depth_limit, int32_t* order);
/* the device's shared single-precision functions on arrays: mode 0 atan2f(a, b), 1 hypotf(a, b), 2 sinf(a), 3 cosf(a) */
int alego_debug_math(alego_handle* h, int mode, const float* a, const float* b, float* out, int n);
/* The four cost functors of include/alego/utility.h:122-349 evaluated on the device exactly as the solvers evaluate them
 * (csrc/dev_cost.h): type 0 SurfCostFunction, 1 CornerCostFunction, 2 LidarEdgeCostFunction, 3 LidarPlaneCostFunction;
 * geom13[i] = cp(3), lpj | normal(3), lpl(3), lpm(3), negative_OA_dot_norm; out: res[i], jac6[i][6] */
int alego_debug_eval_blocks(alego_handle* h, int type, int n, const double* geom13, const double* params6, double* res, double* jac6);
/* transformToStart (laserOdometry.cpp:728-740) of n points with LaserOdometry params_ = params6, as lo_assoc applies it */
int alego_debug_transform_to_start(alego_handle* h, const double* params6, const alego_point* pts, int n, alego_point* out);
/* development aid: with ALEGO_DEBUG_CANARY=1 in the environment every device allocation of the library is framed by 4 KB guard
 * pages of a known pattern; returns how many allocations have a damaged guard (0 = none, -1 = guards not enabled) and describes
 * them in `report` */
int alego_debug_check_guards(char* report, int cap);
/* Run-time switches of kernel variants (parity tests run both variants of a kernel inside one process).  Read once from
 * the environment at alego_create (ALEGO_CC_FUSED, ALEGO_FE_PICK1, ALEGO_LO_BOX_LDS, ALEGO_MAP_MERGE, ALEGO_LM_TOTAL_MERGE, ALEGO_IP_FAST); this
 * call overrides one of them by its environment name.  Not a hot-path call. */
int alego_debug_set_option(alego_handle* h, const char* name, int value);

/* ---- key-frame pass-through for a host-side pose graph (laserMapping.cpp:491-596) -------------------------------
 * LaserMapping keeps the recent_keyframe_num newest key frames of every slot on the device: the down-sampled clouds as
 * saveKeyFramesAndFactor stores them (corner_frames_ / surf_frames_ / outlier_frames_, sensor frame, :553-555) and the
 * f32 key pose (cloud_keyposes_6d_, :531-537).  A host pose graph (GTSAM in the reference) reads every new key frame
 * when ALEGO_FLAG_LM_KEYFRAME is returned, and writes corrected poses back after a loop closure. */
typedef struct alego_keyframe {
  int32_t id;            /* index in cloud_keyposes_3d_ (0-based); the reference's intensity field is id + 0.1 (:529) */
  float pose[6];         /* x y z roll pitch yaw (PointXYZIRPYT, utility.h:83-92) */
  alego_point* corner;   int32_t corner_cap;   int32_t n_corner;   /* laser_corner_ds_  of the frame (may be NULL) */
  alego_point* surf;     int32_t surf_cap;     int32_t n_surf;     /* laser_surf_ds_ */
  alego_point* outlier;  int32_t outlier_cap;  int32_t n_outlier;  /* laser_outlier_ds_ */
} alego_keyframe;
/* number of key frames saved so far by `slot` (cloud_keyposes_3d_->size()) */
int alego_lm_keyframe_count(alego_handle* h, int slot);
/* copy key frame kf_id (-1 = the newest) to the host; only the recent_keyframe_num newest ones are resident
 * (older ids return ALEGO_ERR_ARG: the host keeps its own copy, as the reference does).  publish() (:586-596) is the
 * `pose` of every frame. */
int alego_lm_get_keyframe(alego_handle* h, int slot, int kf_id, alego_keyframe* out);
/* correctPoses (:569-578): overwrite the key pose of a resident frame; the device re-transforms its clouds.  The local
 * map is rebuilt at the next mapping frame once alego_lm_reset_window has been called (the reference clears the
 * recent_* deques at :563-565 and refills them from the newest frames at :208-223). */
int alego_lm_set_keypose(alego_handle* h, int slot, int kf_id, const float pose6[6]);
int alego_lm_reset_window(alego_handle* h, int slot);
/* correctPoses (:579-580): q_map2odom <- R q_map2odom, t_map2odom <- R t_map2odom + c, with the row-major 3x4 [R | c] */
int alego_lm_apply_correction(alego_handle* h, int slot, const double rc[12]);
/* push_back a key frame from host data (clouds in the sensor frame + pose): restores a saved session or lets the host
 * pose graph insert a frame; equivalent to :531-555 with the given pose and clouds.  The device keeps the recent_keyframe_num + 1
 * newest frames.  A FULL window only advances by one frame per mapping frame (:224-237) and so falls behind the newest frames by
 * one for every extra frame inserted; it may lag by one.  An insertion that would make it lag further returns ALEGO_ERR_CAPACITY —
 * call alego_lm_reset_window first when inserting in bulk (the window is then rebuilt from the newest frames, :208-223). */
int alego_lm_add_keyframe(alego_handle* h, int slot, const float pose6[6], const alego_point* corner, int32_t n_corner,
                          const alego_point* surf, int32_t n_surf, const alego_point* outlier, int32_t n_outlier);

/* ---- the global map (saveMapCB, laserMapping.cpp:826-874; visualizeGlobalMapThread, :598-631) -----------------------------
 * The device keeps only the recent_keyframe_num + 1 newest key frames.  The opt-in ARCHIVE keeps every key frame of every slot on the
 * device — its sensor-frame clouds exactly as the ring stores them (after any kf_cap_* truncation) and its f32 key pose — appended by a
 * kernel behind the key-frame store on the slot's own stream, so the batch path needs no host synchronisation per scan (the key-frame
 * counterpart of alego_trajectory_enable).  The map is re-assembled from the archive at the poses that hold NOW, as the reference does
 * after correctPoses (:561-584) rewrote them.
 *
 * alego_map_enable: capacities per slot (device memory: max_points * 16 B + max_keyframes * 56 B + 4 B per slot).  Call it once, before the
 * first key frame is saved; a second call, a call after key frames exist and a call on a handle set up with alego_stream_setup return
 * ALEGO_ERR_ARG.  A frame that does not fit is dropped whole and counted, and so is every later frame: the archived frames are always
 * the prefix 0 .. frames stored - 1 of the key-frame ids.  alego_lm_add_keyframe appends too; alego_lm_set_keypose also updates the
 * archived pose of the frame.  Every other alego_map_* call returns ALEGO_ERR_ARG while the archive is off.
 * alego_map_status: out = {frames stored, frames dropped, points stored, point capacity}.
 * alego_map_set_keyposes: correctPoses (:569-578) over the whole graph: poses6[n][6] (x y z roll pitch yaw) of archived frames
 *   first .. first + n - 1.  It does not touch the resident ring (resident frames still go through alego_lm_set_keypose).
 * alego_map_get_keyframe: any archived frame, as alego_lm_get_keyframe returns a resident one.
 * alego_map_get_stamps / alego_map_set_stamps: the stamps of archived frames first .. first + n - 1 (detectLoopClosure's key-pose time,
 *   :782).  A frame saved by a scan of alego_scan_process, or of alego_lo_process + alego_lm_process (alego_seg_out.stamp), carries
 *   that scan's stamp.  The batch and replay paths carry no stamps: there a frame's stamp is (m - 1) * scan_period, with m the slot's
 *   mapping frames so far (scans with odometry) when it was saved.  alego_lm_add_keyframe stamps by the same rule.  Hosts that know
 *   the true stamps, or that restore a session, overwrite them with alego_map_set_stamps. */
int alego_map_enable(alego_handle* h, int32_t max_keyframes, int32_t max_points);
int alego_map_get_stamps(alego_handle* h, int slot, int32_t first, int32_t n, double* out);
int alego_map_set_stamps(alego_handle* h, int slot, int32_t first, int32_t n, const double* stamps);
int alego_map_status(alego_handle* h, int slot, int32_t out[4]);
int alego_map_set_keyposes(alego_handle* h, int slot, int32_t first, int32_t n, const float* poses6);
int alego_map_get_keyframe(alego_handle* h, int slot, int32_t id, alego_keyframe* out);
/* kinds of alego_map_assemble */
enum {
  ALEGO_MAP_SURF = 1,
  ALEGO_MAP_CORNER = 2,
  ALEGO_MAP_OUTLIER = 4,
  ALEGO_MAP_FRAME_ID = 8   /* intensity = frame index (transformPointCloud(cloud, pose, idx), laserMapping.h:178-186; saveMapCB :844-852) */
};
/* The global map of `slot`: archived frames in id order, each transformed by its archived key pose (transformPointCloud,
 * laserMapping.h:164-177), within a frame surf, corner, outlier restricted to `kinds` (:607-612).  saveMapCB's corner.pcd is
 * kinds = CORNER | FRAME_ID (surf.pcd, outlier.pcd likewise); the /laser_cloud_surround cloud is SURF | CORNER | OUTLIER.
 * leaf > 0: the concatenation goes through pcl::VoxelGrid(leaf) (as alego_voxel_grid) before the copy-out; leaf <= 0: the raw
 * concatenation, which is what saveMapCB writes.  Returns the number of points; out == NULL with cap == 0 only counts; a cap smaller
 * than the count returns ALEGO_ERR_CAPACITY and writes nothing. */
int alego_map_assemble(alego_handle* h, int slot, int kinds, float leaf, alego_point* out, int32_t cap);
/* saveMapCB's keypose.pcd (:833-838): xyz of every archived frame's key pose, intensity = index.  Returns the count (out == NULL with
 * cap == 0 only counts). */
int alego_map_keyposes(alego_handle* h, int slot, alego_point* out, int32_t cap);
/* corner_from_map_ds_ / surf_from_map_ds_ of the last mapping frame of `slot` (the local map visualizeGlobalMapThread publishes on
 * /recent_keyframes, :618-628); n_out = {corner points, surf points}; either buffer may be NULL (count only). */
int alego_lm_get_local_map(alego_handle* h, int slot, alego_point* corner, int32_t corner_cap, alego_point* surf, int32_t surf_cap, int32_t n_out[2]);
/* pcl::VoxelGrid<PointXYZI>::filter(leaf) of a host cloud of any size (f32 getMinMax3D, the dx dy dz > INT_MAX "leaf size too small"
 * rule that returns the input unchanged, PCL's 32-bit voxel index, stable order inside a voxel, f32 sums in input order divided by the
 * count), bit-exact.  Small clouds go to the one-workgroup kernels of the local maps, large ones to a multi-kernel radix sort spread
 * over the whole device.  leaf must be > 0.  Returns the number of voxels (out == NULL with cap == 0 only counts);
 * ALEGO_ERR_CAPACITY when cap is too small (nothing written).  Scratch grows with the largest n seen and stays with the handle. */
int alego_voxel_grid(alego_handle* h, const alego_point* pts, int32_t n, float leaf, alego_point* out, int32_t cap);
/* pcl::io::savePCDFile's product as PCD v0.7, DATA binary, FIELDS x y z intensity (F 4 each), WIDTH n, HEIGHT 1, VIEWPOINT 0 0 0 1 0 0 0
 * (saveMapCB :869-872).  Host only.  0 or ALEGO_ERR_ARG (bad arguments, the file cannot be written). */
int alego_write_pcd(const char* path, const alego_point* pts, int32_t n);

/* ---- loop closure (laserMapping.cpp:633-824): the host keeps the pose graph (GTSAM in the reference) and every key frame; the
 * library does the per-point work of one closure attempt.
 *   alego_loop_detect        detectLoopClosure's choice (:771-790), plain host code: the key pose nearest to `cur_xyz` within
 *                            lc_search_radius whose stamp is more than lc_min_time_gap older than the newest key frame's; -1 = none
 *   alego_loop_closure_icp   sub-map assembly (:794-812: the newest key frame as ICP source; the history frames
 *                            closest - lc_search_num .. closest + lc_search_num, transformed by their key poses, concatenated and
 *                            VoxelGrid(lc_leaf)-filtered as target) and pcl::IterativeClosestPoint as configured at :670-692.
 *                            `correction` = getFinalTransformation() (row-major 4x4, f32), `fitness` = getFitnessScore().  The caller
 *                            applies :697 (converged && fitness <= lc_fitness_max), adds the Between factor (:716-733) and, after the
 *                            graph update, writes the corrected poses back (alego_lm_set_keypose / reset_window / apply_correction).
 *                            target_out (may be NULL): near_history_keyframes_ for /history_keyframes. */
typedef struct alego_kf_in {
  float pose[6];                                   /* x y z roll pitch yaw of the key frame */
  const alego_point* corner;   int32_t n_corner;   /* corner_frames_[id], surf_frames_[id], outlier_frames_[id] (sensor frame) */
  const alego_point* surf;     int32_t n_surf;
  const alego_point* outlier;  int32_t n_outlier;
} alego_kf_in;
typedef struct alego_icp_result {
  int32_t converged, iterations, n_source, n_target;
  double fitness;
  float correction[16];
} alego_icp_result;
int alego_loop_detect(const alego_params* params, const float* keyposes6, const double* stamps, int32_t n, const double cur_xyz[3]);
int alego_loop_closure_icp(alego_handle* h, const alego_kf_in* latest, const alego_kf_in* history, int32_t n_history,
                           alego_icp_result* out, alego_point* target_out, int32_t target_cap);

/* ---- batched loop-closure search over the key-frame archive (needs alego_map_enable)
 *   alego_loop_search        performLoopClosure + detectLoopClosure (:652-824) for every listed slot at once, from the archive: the
 *                            current position is the slot's t_map2laser_ (alego_batch_get_pose's map pose) as f32; detection as
 *                            alego_loop_detect on the archived key poses and stamps; source = the newest archived frame (surf,
 *                            corner, outlier); target = frames closest ± lc_search_num below the newest, transformed by their archived
 *                            poses and VoxelGrid(lc_leaf)-filtered; ICP as alego_loop_closure_icp.  out[i] belongs to slots[i].
 *                            Synchronous; it runs behind the work already queued on every stream group and changes no device state
 *                            (archive, poses, window): the host adds the Between factor to its graph and writes corrected poses back
 *                            (alego_map_set_keyposes, alego_lm_set_keypose, alego_lm_reset_window, alego_lm_apply_correction).
 *                            A slot's result does not depend on the other slots of the call.  ALEGO_ERR_ARG with the archive off or
 *                            a slot out of range.
 *   alego_loop_constraint    host only: t_correct and between from an ICP correction and the two key poses (:714-730), as
 *                            alego_loop_search fills them in. */
typedef struct alego_loop_result {
  int32_t status;          /* 0 no candidate (or no key frame), 1 attempted and rejected (:697), 2 accepted, < 0 slot not searchable
                              (-1: its archive dropped frames) */
  int32_t latest_id, closest_id;
  int32_t converged, iterations, n_source, n_target;
  double fitness;          /* getFitnessScore() */
  float correction[16];    /* getFinalTransformation(), row-major */
  float t_correct[16];     /* correction * initial_guess (:714-715; initial_guess = the newest key pose, :680-687) */
  double between[12];      /* pose_from.between(pose_to), row-major [R | t]: the BetweenFactor measurement (:716-730) */
  double noise_variance;   /* (float)fitness: the diagonal Variances of constraint_noise_ (:724-728) */
} alego_loop_result;
int alego_loop_search(alego_handle* h, const int32_t* slots, int32_t n, alego_loop_result* out);
int alego_loop_constraint(const float correction[16], const float latest_pose6[6], const float closest_pose6[6],
                          float t_correct[16], double between12[12]);
/* the exact 1-NN of alego_loop_search on its own (tests): for every query the target index with the smallest f32 squared distance
 * ((dx dx + dy dy) + dz dz), the lowest index on ties; idx = -1, d2 = FLT_MAX for an empty target or a non-finite query */
int alego_debug_nn1(alego_handle* h, const alego_point* tgt, int32_t n_tgt, const alego_point* queries, int32_t n_q, int32_t* idx, float* d2);

/* ---- the key-pose graph (saveKeyFramesAndFactor :491-559, correctPoses :561-584, the Between factor of :716-733), kept per slot next to
 * the key-frame archive and optimised on the device (needs alego_map_enable)
 *   nodes     the archived key frames 0 .. N-1 of a slot as Pose3
 *   prior     on node 0 (:495): key pose 0 as it was archived
 *   odometry  edge i-1 -> i for every later frame (:510-512): between(pose[i-1], pose[i]) in f64, both poses Pose3(Rot3::RzRyRx(roll, pitch,
 *             yaw), xyz) of the ARCHIVED f32 key poses — pose[i-1] as it stands when frame i is appended (the reference's pre_pose, :500)
 *             and pose[i] the new frame's f32 pose (the reference uses the f64 q/t_map2laser_ there; the f32 image is what it stores and
 *             what alego_lm_add_keyframe knows, and the difference is below f32 rounding of the pose).  Recorded by the archive's kernel.
 *   loops     edge from -> to with a measured Pose3 and six variances, added by the host from alego_loop_search / alego_loop_closure_icp
 *   noise     diagonal variances per edge in GTSAM's tangent order: rotation x y z, then translation x y z.  The default of the prior and
 *             the odometry is {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6} (:68-70) — in that order the two 1e-8 entries weigh translation x and
 *             y; the quirk is kept.
 *   error     Logmap(measured^-1 (x_from^-1 x_to)), prior: Logmap(prior^-1 x_0), with the full SE(3) Logmap (GTSAM_POSE3_EXPMAP /
 *             GTSAM_ROT3_EXPMAP, GTSAM's default since 4.0.3); update x <- x Expmap(delta)
 * alego_graph_optimize computes the MINIMISER of the sum of squared whitened errors by plain Gauss-Newton in f64 (no damping), started
 * from the archived poses as they are now.  iSAM2 as the reference drives it (relinearizeSkip 1, two update() calls per factor) takes
 * Gauss-Newton steps towards the same point without iterating to it: the contract here is the optimum, not iSAM2's iterate. */
#define ALEGO_GRAPH_MAX_LOOPS 64   /* largest max_loops of alego_graph_enable */
typedef struct alego_graph_edge {
  int32_t from, to;        /* from = -1: the prior on node `to` (between = the prior pose) */
  double between[12];      /* the measurement, row-major 3x4 [R | t] */
  double variance[6];      /* rotation x y z, translation x y z */
} alego_graph_edge;
/* Once, after alego_map_enable and before the first key frame (else ALEGO_ERR_ARG).  max_loops in [1, ALEGO_GRAPH_MAX_LOOPS]: loop edges a slot
 * can hold.  odom_variance: of the prior and of every recorded odometry edge; NULL = the default above.  Device memory per slot:
 * max_keyframes * (152 + 96) B + max_loops * 152 B + 80 B.  Without this call nothing of the graph is allocated or launched. */
int alego_graph_enable(alego_handle* h, int32_t max_loops, const double odom_variance[6]);
/* out = {chain edges (one per archived frame), loop edges stored, loop_closed_ (a loop edge was added since the last apply), poses of
 * the estimate of the last optimise} */
int alego_graph_status(alego_handle* h, int slot, int32_t out[4]);
/* edges first .. first + n - 1 of `slot`: kind 0 the chain (edge 0 is the prior, edge i the odometry edge i-1 -> i; one per archived frame),
 * kind 1 the loop edges in the order they were added */
int alego_graph_get_edges(alego_handle* h, int slot, int kind, int32_t first, int32_t n, alego_graph_edge* out);
/* overwrite chain edges first .. first + n - 1 (restored sessions, as alego_map_set_stamps): chain[j] must be the prior (from -1, to 0) or
 * first + j - 1 -> first + j.  alego_lm_set_keypose / alego_map_set_keyposes never touch edges: a measurement stays what was measured. */
int alego_graph_set_edges(alego_handle* h, int slot, int32_t first, int32_t n, const alego_graph_edge* chain);
/* append, for every r[i] with status == 2, the edge latest_id -> closest_id with r[i].between and r[i].noise_variance on all six components
 * (:716-733) to slots[i]; r[i].correction is kept as the slot's map -> odom correction (:734).  Sets the slot's loop_closed_.
 * alego_graph_add_edge: one edge from any source (e.g. alego_loop_closure_icp); correction = row-major 4x4, NULL = identity.
 * ALEGO_ERR_ARG: graph off, slot out of range, ids outside [0, frames stored), from == to, a variance not positive and finite, a
 * measurement not finite.  ALEGO_ERR_CAPACITY: max_loops edges are stored already.  On any error nothing is written. */
int alego_graph_add_loops(alego_handle* h, const int32_t* slots, int32_t n, const alego_loop_result* r);
int alego_graph_add_edge(alego_handle* h, int slot, const alego_graph_edge* e, const float correction[16]);
/* Defaults (opts == NULL, or a field <= 0): max_iters = ALEGO_GRAPH_MAX_ITERS, step_tol = ALEGO_GRAPH_STEP_TOL, apply = 0.
 * Observed on the MI355X over the constructed graphs of tests/test_pose_graph.py (drifted circles of 2 .. 2000 poses, up to 19 m / 0.34 rad
 * of end drift, 1 .. 64 loop edges of variance 1e-4 .. 0.4; table in DESIGN.md section 13): the step shrinks 10 - 100 x per iteration
 * (linearly: the loop residual does not vanish at the optimum).  Steps until the largest component is below 1e-9: 2 (2 and 3 poses), 6 - 7
 * (150 poses, 1 - 8 loop edges; 2000 poses), 10 in the worst case (400 poses, 18.7 m / 0.27 rad), hence max_iters = 2 x 10.  Left to run,
 * the steps stagnate between 6e-17 and 2.0e-13 (largest on 2000 poses), so step_tol = 1e-9 is 5000 x above the stagnation level; with it
 * the estimate ends within 2.7e-11 m / 8.8e-13 rad of the optimum.  The test asserts both margins on the device. */
#define ALEGO_GRAPH_MAX_ITERS 20
#define ALEGO_GRAPH_STEP_TOL 1e-9
typedef struct alego_graph_opts {
  int32_t max_iters;       /* Gauss-Newton steps at most */
  double step_tol;         /* stop when the largest component of delta (rad, m) is below it */
  int32_t apply;           /* 1: correctPoses (:561-584) on the device for every slot that converged and has had a loop edge added since its last apply */
} alego_graph_opts;
typedef struct alego_graph_result {
  int32_t status;          /* 2 converged, 1 max_iters reached (not applied), 0 no key frame, -1 the archive dropped frames, -2 a step was not finite
                              (the slot's poses and estimate are left untouched) */
  int32_t iterations, n_poses, n_loops, applied;
  double cost0, cost;      /* sum of squared whitened errors at the archived poses / at the estimate (the first Gauss-Newton step of a drifted
                              loop RAISES the cost before it falls: only cost <= cost0 at the end holds) */
  double last_step;        /* largest |component| of the last delta */
} alego_graph_result;
/* Optimise the graphs of the listed slots at once; out[i] belongs to slots[i].  Synchronous; runs behind the work already queued on every stream
 * group.  A slot's result does not depend on the other slots of the call, their order or the chunking (sums run in a fixed order).
 * ALEGO_ERR_ARG: graph off, a slot out of range or listed twice.
 * apply = 1: archived poses <- f32 (x y z, roll = atan2(R21, R22), pitch = atan2(-R20, sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00)) of the
 * estimate; the resident key frames get the same poses and are re-transformed; the local-map window is reset as by alego_lm_reset_window;
 * map -> odom is corrected by the LAST loop edge's correction as by alego_lm_apply_correction; loop_closed_ is cleared — the same state the
 * per-slot calls alego_map_set_keyposes + alego_lm_set_keypose (every resident frame) + alego_lm_reset_window + alego_lm_apply_correction
 * leave, without a host call or a synchronisation per slot. */
int alego_graph_optimize(alego_handle* h, const int32_t* slots, int32_t n, const alego_graph_opts* opts, alego_graph_result* out);
/* poses first .. first + n - 1 of the f64 estimate of the slot's last optimise with status > 0, row-major 3x4 each */
int alego_graph_get_estimate(alego_handle* h, int slot, int32_t first, int32_t n, double* poses12);
/* host only (csrc/pg_math.h, the arithmetic the kernels run): whitened errors [n_edges][6] and the Jacobian blocks d error / d delta_from,
 * d error / d delta_to [n_edges][36] (row-major; zero for the `from` side of a prior) of `edges` over poses12[n_poses][12]; any output may be NULL */
int alego_graph_residuals(const double* poses12, int32_t n_poses, const alego_graph_edge* edges, int32_t n_edges,
                          double* whitened6, double* jac_from36, double* jac_to36);

/* ---- marginal covariances of the key-pose graph and a gate for candidate loop edges (what gtsam::Marginals gives a
 * GTSAM user).  Linearisation point: the slot's archived key poses as they stand now, as Pose3 — where alego_graph_optimize starts; after an
 * optimise with apply = 1 that is the optimum to f32 rounding.  Covariances are GTSAM's: tangent space of the pose, right perturbation
 * (x <- x Expmap(delta)), rotation first; row-major 6x6, symmetric to the last bit.
 * The device calls are synchronous, run behind the work queued on every stream group (as alego_graph_optimize) and change nothing of a slot:
 * poses, estimate, loop_closed_ and edges all stay; nothing is kept on the device.  A slot's outputs do not depend on the other slots of the
 * call, their order or the chunking.  ALEGO_ERR_ARG with the graph off (so on a localising handle too).  Without a call nothing is allocated
 * or launched.
 * Gate: for a candidate from -> to with measurement and variances, d2 = e^T P^-1 e with e the unwhitened error Logmap(measured^-1 (x_from^-1
 * x_to)) and P = the covariance of e the graph predicts + diag(variance); compare d2 with a chi-square quantile of 6 degrees of freedom.
 * NOTE on noise: with the default odometry variances (1e-6 / 1e-8) the graph claims millimetres of drift over a lap and the gate refuses every
 * real loop.  A host that gates either passes honest odometry variances to alego_graph_enable, or lets the library measure them: with
 * alego_regcov_enable (opts.graph = 1, below) every odometry edge carries the variances of the registration that produced its frame. */
#define ALEGO_GRAPH_CHI2_6_999 22.457744484825323   /* chi-square, 6 dof, 0.999 */
typedef struct alego_graph_cov_result { int32_t status, n_poses, n_loops, pad; } alego_graph_cov_result;
   /* status: 1 computed, 0 no key frame, -1 the archive dropped frames, -2 not finite */
/* cov36: [n][cap][36] row-major, poses 0 .. min(n_poses, cap) - 1 of slots[i] (the rest of a slot's rows is left as it was).
 * ALEGO_ERR_ARG: a slot out of range or listed twice, cap <= 0, a null argument. */
int alego_graph_marginals(alego_handle* h, const int32_t* slots, int32_t n, int32_t cap, double* cov36, alego_graph_cov_result* out);
typedef struct alego_graph_check {
  int32_t status, pad;     /* 1 computed, 0 not judged (alego_graph_check_loops: r[i].status != 2), -1 the archive dropped frames, -2 P not finite or
                              not positive definite (d2 = 0) */
  double d2;               /* squared Mahalanobis distance */
  double error[6];         /* e, rotation first */
  double cov[36];          /* P */
} alego_graph_check;
/* candidate e[i] for slots[i]; a slot may be listed several times (at most ALEGO_GRAPH_MAX_LOOPS candidates per slot and call, else
 * ALEGO_ERR_CAPACITY); every candidate is judged against the same graph, independently of the others.  Same argument errors as alego_graph_add_edge. */
int alego_graph_check_edges(alego_handle* h, const int32_t* slots, int32_t n, const alego_graph_edge* e, alego_graph_check* out);
/* the edge alego_graph_add_loops would append for r[i] (status == 2; others give status 0) */
int alego_graph_check_loops(alego_handle* h, const int32_t* slots, int32_t n, const alego_loop_result* r, alego_graph_check* out);
/* host only, the same arithmetic (csrc/pg_cov_math.h): marginals [n_poses][36] and, for pairs[n_pairs][2] = (i, j), Sigma_ij [n_pairs][36] (rows of
 * node i, columns of node j); edges: the n_poses chain edges first (edge 0 the prior, edge k: k - 1 -> k), then the loop edges; any output may be
 * NULL.  ALEGO_ERR_ARG: a null input, a malformed edge list, ids out of range, from == to, a variance not positive and finite, values not finite. */
int alego_graph_covariance_host(const double* poses12, int32_t n_poses, const alego_graph_edge* edges, int32_t n_edges,
                                const int32_t* pairs, int32_t n_pairs, double* marg36, double* pair36);
int alego_graph_check_host(const double* poses12, int32_t n_poses, const alego_graph_edge* edges, int32_t n_edges,
                           const alego_graph_edge* cand, int32_t n_cand, alego_graph_check* out);

/* ---- covariance and degeneracy of LaserMapping's scan-to-map registration (csrc/reg_cov_math.h) -----------------
 * Opt-in per handle; without alego_regcov_enable nothing is allocated or launched.  With it, every mapping frame of every slot that registers
 * (SLAM and localising handles alike) leaves one record, computed on the device between the solver and the key-frame decision from ONE full
 * evaluation of the accepted rows at the solver's final point p = (x, y, z, roll, pitch, yaw): H = J^T J (Huber-corrected as the solver
 * forms it), J^T r and the cost 1/2 sum rho.
 *   info      N^T H N, N = M^-1, xi = M dp the pose's tangent vector in GTSAM's convention (right perturbation, rotation x y z first, then
 *             translation x y z — the space of alego_graph_edge.variance and alego_graph_marginals)
 *   eigval    of info, ascending (ties by index), eigvec column k the unit vector of eigval[k] (cyclic Jacobi, f64)
 *   n_degenerate   eigenvalues below eig_min (LOAM / LeGO-LOAM's isDegenerate; default 100 = LeGO-LOAM's eignThre, a parameter)
 *   sigma2    max(sigma0^2, 2 cost / (rows - 6)): the residual variance, floored by the sensor's sigma0 (default 0.02 m)
 *   cov       sigma2 V diag(1 / max(eigval_k, lambda_rel_floor eigval_max)) V^T, symmetric to the last bit
 *   variance  clamp(scale cov[k][k], var_min[k], var_max[k]); defaults: scale 1, lambda_rel_floor 1e-12, var_max 1 (rad^2, m^2), var_min = the
 *             odometry variances of alego_graph_enable when the graph is on at the time of the call, else its default {1e-6 x 3, 1e-8 x 2, 1e-6}
 * All of these are parameters of a noise model, not measurements.  Query points are f32 on the device, everything else f64.
 * opts.graph = 1 (needs alego_graph_enable before this call): the odometry edge map_archive records for a key frame carries `variance` of
 * that frame's record when its status is 1; the prior, a frame inserted by alego_lm_add_keyframe and any other status keep odom_variance.
 * Model: the edge's noise is the registration covariance of the NEWER frame alone, read in its own tangent space — at zero error the
 * Jacobian of the between-error with respect to the `to` pose is the identity — and diagonal (alego_graph_edge holds six variances); the
 * correlation with the older frame through the shared local map is ignored.
 * Not available with a sharded registration: alego_regcov_enable returns ALEGO_ERR_ARG after alego_dist_init, and alego_dist_init after it. */
typedef struct alego_regcov_opts {
  double sigma0, scale, eig_min, lambda_rel_floor;
  double var_min[6], var_max[6];
  int32_t graph, pad;
} alego_regcov_opts;
typedef struct alego_regcov {
  int32_t status;          /* 1 computed, 0 no registration in the slot's last mapping frame or fewer than 7 rows, -2 not finite, -3 |cos pitch| too small;
                              with a status other than 1 every double below is 0 */
  int32_t n_edge, n_plane, n_degenerate, frame, pad;   /* frame: the slot's mapping-frame counter (lm_info LI_FRAME) the record belongs to */
  double cost, sigma2, info[36], eigval[6], eigvec[36] /* column k = vector of eigval[k] */, cov[36], variance[6];
} alego_regcov;
/* once, before the first scan reaches LaserMapping in any slot, else ALEGO_ERR_ARG; NULL or a field <= 0 = defaults; ALEGO_ERR_ARG also for a
 * field that is not finite, var_min[k] > var_max[k], graph = 1 without the graph, a sharded handle */
int alego_regcov_enable(alego_handle* h, const alego_regcov_opts* opts);
/* the records of the listed slots as the last mapping frame left them (status 0 before the first); synchronous, one copy for the whole list.
 * ALEGO_ERR_ARG: feature off, a null argument, a slot out of range or listed twice */
int alego_regcov_get(alego_handle* h, const int32_t* slots, int32_t n, alego_regcov* out);
/* host twin of the kernel's 6x6 part (the same arithmetic, csrc/reg_cov_math.h): acc28 = upper triangle of H (21, row by row), J^T r (6), cost;
 * var_min defaults to the graph's default odometry variances; frame = 0.  Returns 0, or ALEGO_ERR_ARG for a null argument / bad options */
int alego_regcov_host(const double acc28[28], const double params6[6], int32_t n_edge, int32_t n_plane, const alego_regcov_opts* opts, alego_regcov* out);
/* host: eval_block + accumulate_block (csrc/solve_rows.h) over rows (a, b, p | n, d, p), edges then planes, summed in row order */
int alego_regcov_normal_host(const double params6[6], const double* edge_rows9, int32_t n_edge, const double* plane_rows7, int32_t n_plane, double huber, double acc28[28]);
/* the kernel alone on given rows (p rounded to f32, as the device keeps query points), as alego_debug_eval_blocks is for the functors: the
 * handle's Huber delta, its options when the feature is on and the defaults otherwise; touches no slot */
int alego_debug_regcov(alego_handle* h, const double params6[6], const double* edge_rows9, int32_t n_edge, const double* plane_rows7, int32_t n_plane, alego_regcov* out);

/* ---- solution remapping: LaserMapping's registration holds degenerate directions at its start (csrc/remap_math.h) ----
 * Opt-in per handle (SLAM and localising handles alike); without alego_remap_enable nothing is allocated or launched and lm_solve runs as it
 * always did.  With it the solver kernel of a mapping frame is lm_solve_remap: from the 28 sums of its own first evaluation, at the point x0 the
 * first outer solve starts from — params_ on entry, which is what the slot's last mapping frame left there (the reference's ceres problem
 * keeps optimising one persistent params_; transformAssociateToMap's odometry prediction selects the map, it does not re-seed the solver) — it forms
 *   info      N^T H N, N = M(x0)^-1 — the tangent space of alego_regcov above, so a direction held here is one alego_regcov would count
 *   eigval    of info, ascending (ties by index), eigvec column k the unit vector of eigval[k] (the same cyclic Jacobi)
 *   n_held    eigenvalues below eig_min (default 100, LeGO-LOAM's eignThre)
 *   proj      P = N (sum over the kept k of v_k v_k^T) M, row-major, in PARAMETER space (x, y, z, roll, pitch, yaw); the exact identity when
 *             nothing is held, exactly zero when everything is
 * and every step of every iteration of every outer solve of that frame is replaced by S^-1 P S step (S the solver's Jacobi scaling) before the
 * model cost change is formed: the cost change, the candidate, the step-size and the cost-change tests see the projected step; stopping rules,
 * radius updates and the handling of invalid steps are unchanged, except that a projected step that is exactly zero (everything held) is not
 * invalid — the candidate is the start, and the solve ends by the step-size test (termination 2) with the pose at x0.  A frame with
 * n_held = 0 is solved bit for bit as without the mode.  Zhang, Kaess, Singh, "On degeneracy of optimization-based state estimation problems"
 * (ICRA 2016); LOAM and LeGO-LOAM decide at iterCount == 0 likewise.
 * Independent of alego_regcov_enable (both may be on: alego_regcov reports the final point as before).  Not available with a sharded
 * registration: alego_remap_enable returns ALEGO_ERR_ARG after alego_dist_init, and alego_dist_init after it. */
typedef struct alego_remap_opts {
  double eig_min;          /* <= 0: the default */
} alego_remap_opts;
typedef struct alego_remap {
  int32_t status;          /* 1 computed, 0 no registration in the slot's last mapping frame or fewer than 7 rows, -2 not finite, -3 |cos pitch| too small;
                              with a status other than 1 nothing is held and every double below but `start` is 0 */
  int32_t n_held, frame, pad;   /* frame: the slot's mapping-frame counter (lm_info LI_FRAME) the record belongs to */
  double start[6] /* x0 */, eigval[6], eigvec[36] /* column k = vector of eigval[k] */, proj[36];
} alego_remap;
/* once, before the first scan reaches LaserMapping in any slot, else ALEGO_ERR_ARG; NULL or eig_min <= 0 = the default; ALEGO_ERR_ARG also for an
 * eig_min that is not finite and for a sharded handle */
int alego_remap_enable(alego_handle* h, const alego_remap_opts* opts);
/* the records of the listed slots as the last mapping frame left them (status 0 before the first); synchronous, one copy for the whole list.
 * ALEGO_ERR_ARG: feature off, a null argument, a slot out of range or listed twice */
int alego_remap_get(alego_handle* h, const int32_t* slots, int32_t n, alego_remap* out);
/* host twin of the kernel's 6x6 part (the same functions in the same order, csrc/remap_math.h): acc28 as for alego_regcov_host, params6 = x0;
 * frame = 0.  Returns 0, or ALEGO_ERR_ARG for a null argument / a negative count / an eig_min that is not finite */
int alego_remap_host(const double acc28[28], const double params6[6], int32_t n_edge, int32_t n_plane, const alego_remap_opts* opts, alego_remap* out);
/* host twin of one step of the solver (lm_step, csrc/solve_rows.h) at x = 0: H21 the upper triangle of J^T J row by row, g6 = J^T r, scale6 the
 * Jacobi scaling, radius the trust-region radius, proj36 = P or NULL (the plain step).  step6: the step in parameter space (the candidate),
 * *mcc: the model cost change.  Returns 1 for a valid step, 0 for an invalid one (step6 and *mcc are then 0), ALEGO_ERR_ARG for a null argument */
int alego_remap_step_host(const double H21[21], const double g6[6], const double scale6[6], double radius, const double* proj36, double step6[6], double* mcc);
/* the solver kernel alone on given rows (rows as for alego_debug_regcov, p rounded to f32), from start6: remap = 0 lm_solve, 1 lm_solve_remap with
 * the handle's eig_min (the default while the mode is off); ALEGO_SOLVE_FULL_EVAL selects the _full_eval twin of either; the handle's lm_max_iters,
 * lm_outer_iters and Huber delta.  params_it[2][6], costs[4] (initial / final cost of both solves) and summary[2] (iterations | successful steps
 * << 8 | termination << 16) are what a mapping frame leaves in lm_state and lm_info; rec (may be NULL; zeroed when remap = 0): the record.
 * Touches no slot. */
int alego_debug_remap_solve(alego_handle* h, const double start6[6], const double* edge_rows9, int32_t n_edge, const double* plane_rows7, int32_t n_plane,
                            int32_t remap, double* params_it, double* costs, int32_t* summary, alego_remap* rec);

/* ---- localisation: many streams against ONE frozen key-frame map -------------------------------------
 * A handle-wide mode, off by default (nothing of it is allocated or launched then).  alego_loc_enable hands the handle N key frames — pose
 * and sensor-frame clouds, exactly what alego_map_get_keyframe returns from a mapping run; from then on EVERY slot localises in that map.
 * ImageProjection, feature extraction, LaserOdometry, LaserMapping's gate and laserOdomHandler are unchanged.  A mapping frame of a slot
 *   1  selects its window: p = (float)t_map2laser_ after transformAssociateToMap; frame i is a candidate when its f32 squared distance
 *      ((dx dx) + dy dy) + dz dz to p is < (float)(radius * radius); of the candidates the K = recent_keyframe_num smallest in the order
 *      (d2 bits, id) are kept; the window is their ids in ascending order; a non-finite p selects nothing.  (The project's own rule, not
 *      the reference's surround-key-frame bookkeeping of laserMapping.cpp:245-313.)
 *   2  builds the local map of the window as :238-243 / :315-319 do, in window order — only when the window differs from the last one;
 *   3  runs downsampleCurrentScan, scan2MapOptimization and transformUpdate as they are, with the same guards;
 *   4  never saves a key frame: ALEGO_FLAG_LM_KEYFRAME is never returned, alego_lm_keyframe_count stays 0, the optimised params_ reach
 *      transformUpdate as they are;
 *   5  with an empty window (off the map) down-samples the scan, does not optimise and leaves map -> odom exactly as it was.
 * The initial pose of a slot is set with alego_lm_apply_correction on the fresh slot (map -> odom = [R | c]); params_, from which the
 * first registration starts, with alego_set_lm_params.
 *   alego_loc_select   host only, plain C++: the selection rule above over keyposes6[n][6]; ids ascending, returns their count
 *                      (ALEGO_ERR_ARG for null / negative arguments).  radius <= 0: 50.0.
 *   alego_loc_enable   once, before the first scan of any slot.  radius <= 0: 50.0 (surround_keyframe_search_radius_, LM.cpp:183).
 *                      ALEGO_ERR_ARG: a second call, a call after a scan, with the archive / graph enabled or after alego_stream_setup.
 *                      ALEGO_ERR_CAPACITY (+ alego_last_error): a frame exceeds the handle's key-frame capacities, more than 8192 frames,
 *                      or the store does not fit.  Device memory: 32 * (corner capacity + surf capacity + outlier capacity) + 112 B per
 *                      frame, once per handle; the slots' own key-frame rings are released.
 *   alego_loc_status   out = {map frames, frames in the window of the last mapping frame, local-map rebuilds so far, 1 if that frame optimised}
 *   alego_loc_enable_from_map   alego_loc_enable with the frames taken on the device from the archive of `slot` of the mapping handle `map`
 *                      (same process, same device) as it is NOW: N = its stored frames, frame i = what alego_map_get_keyframe(map, slot, i)
 *                      returns now, i.e. with the poses alego_graph_optimize, alego_map_set_keyposes, _move, _merge or _thin left.  Every
 *                      observable of the handle afterwards is bit-identical to alego_loc_enable on those frames; no frame crosses to the host.
 *                      The frames go through the store in chunks.  Every stream of `map` is synchronised first (a key
 *                      frame queued by alego_batch_run(.., sync = 0) is handed over); then `map` is only read and keeps mapping.  An archive
 *                      that dropped frames hands over its stored prefix.  capacity: frames the store is allocated for; <= 0: N; it sizes the
 *                      memory (below, per frame of capacity) and changes no result.  Preconditions, codes and messages of alego_loc_enable,
 *                      and ALEGO_ERR_ARG: map null, map == h, map without archive, slot out of range of map, handles on different devices;
 *                      ALEGO_ERR_CAPACITY: a frame exceeds h's key-frame capacities (the message names the first one and its counts; decided
 *                      from a host copy of the archive's frame table before anything is allocated), N > 8192, capacity < N or > 8192.  After
 *                      any failure h is the SLAM handle it was.  A store built by alego_loc_enable has capacity max(N, 1).  During the call a
 *                      temporary staging area and sort scratch of at most 256 MiB are held (16 B per point of staging, 20 B per point of
 *                      scratch for a run of more than 8192 points, per frame of a chunk).
 *   alego_loc_update_from_map   on a handle that localises, at any time; synchronous; runs behind the work queued on every stream group of h
 *                      and behind map's.  The WHOLE store is rebuilt from the archive as it is now (N may shrink or grow up to the store's
 *                      capacity), and every slot of h gets what alego_lm_reset_window does to a SLAM slot: its window is emptied, its voxel
 *                      lists and local maps are stale, and its next mapping frame selects in the new map at its own pose and rebuilds.  Map ->
 *                      odom, params_, LaserOdometry's state and the scan counters of every slot stay bit for bit; alego_loc_status reports the
 *                      new frame count at once and window 0 until the slot's next mapping frame.  After alego_reloc_enable the map descriptors
 *                      and ring keys are rebuilt too (their buffers are sized by the store's capacity).  ALEGO_ERR_ARG: h does not localise,
 *                      or a source case of alego_loc_enable_from_map.  ALEGO_ERR_CAPACITY: N exceeds the store's capacity or a frame h's
 *                      key-frame capacities — decided before anything is written, the store is untouched.  A device error in the middle
 *                      returns ALEGO_ERR_HIP and leaves the store EMPTY (0 frames: every slot is off the map and dead-reckons, rule 5) until
 *                      an update succeeds.
 *   A host that drives the handles from several threads holds both handles' locks around either call (alego_handle_lock), map's first.
 *   alego_debug_get names of a localising handle (tests; the slot argument is ignored, <f> is a frame of the store): "ls_corner:<f>" /
 *   "ls_surf:<f>" the sorted corner / surf + outlier run, "ls_box_c:<f>" / "ls_box_s:<f>" their boxes (8 floats), "ls_raw_c:<f>" / "ls_raw_s:<f>" /
 *   "ls_raw_o:<f>" the clouds as stored, "ls_pose:<f>" (8 floats), "ls_counts:<f>" (i32: the two run counts, then corner, surf, outlier points).
 *   alego_debug_set_option("ALEGO_LOC_CHUNK", c) on the localising handle sets the frames per chunk of both calls (default 128).
 * On a localising handle alego_map_enable / alego_graph_enable, every alego_map_* / alego_graph_* call that takes a handle,
 * alego_loop_search, alego_lm_add_keyframe / _set_keypose / _reset_window / _get_keyframe, alego_stream_setup, alego_dist_init and
 * alego_debug_set_option("ALEGO_MAP_MERGE", 0) return ALEGO_ERR_ARG.  alego_debug_get(.., "lm_window") returns the window's map-frame ids;
 * doubles 44..46 of "lm_state" hold p of the last mapping frame. */
int alego_loc_select(const float* keyposes6, int32_t n, const float xyz[3], double radius, int32_t k, int32_t* ids);
int alego_loc_enable(alego_handle* h, const alego_kf_in* frames, int32_t n, double radius);
int alego_loc_enable_from_map(alego_handle* h, alego_handle* map, int slot, double radius, int32_t capacity);
int alego_loc_update_from_map(alego_handle* h, alego_handle* map, int slot);
int alego_loc_status(alego_handle* h, int slot, int32_t out[4]);

/* ---- relocalisation: placing slots of a localising handle without an initial pose ------------------------
 * Place recognition for many slots at once: a rotation-invariant descriptor of every map frame and of a slot's current scan, an EXACT
 * search of the scan's descriptor over all N map frames, verification by the ICP of alego_loop_search.  The rule (csrc/reloc_math.h; the
 * project's own, in the family of Scan Context), all f32 without contraction:
 *   descriptor  60 sectors x 20 rings of one byte, D[sector][ring] (1200 B).  A point with a non-finite coordinate is skipped;
 *               r = sqrtf((x x) + (y y)), w = (float)max_range / 20.0f, ring = floorf(r / w), skipped unless ring < 20;
 *               sector = min(59, floorf((atan2f(y, x) + (float)pi) * (float)(60 / 2 pi))); code = min(255, max(1, floorf((z + z_offset) * 16.0f) + 1));
 *               D[sector][ring] = the largest code of its points, 0 for an empty bin.  ring key: key[ring] = sum over sectors of D[sector][ring] (u16).
 *               A map frame's descriptor is that of its corner, surf and outlier clouds; a slot's that of laser_corner_ds_, laser_surf_ds_ and
 *               laser_outlier_ds_ of its last mapping frame (the clouds a key frame would have been saved from).
 *   match       dist(Q, M, s) = sum over c, r of |Q[(c + s) mod 60][r] - M[c][r]|; D_i = min over s, s_i the smallest s attaining it; the
 *               candidates are the n_cand frames smallest in the order (D_i, i) — exactly the brute force over all frames and shifts.
 *   guess       guess6 = key pose of frame i with yaw - (float)s_i * (float)(2 pi / 60), f32.
 *   verify      candidates in order, at most `verify` of them: source = the slot's three clouds as the frame (guess6, corner, surf, outlier);
 *               target = map frames [i - lc_search_num, i + lc_search_num] within [0, N), each transformed by its pose (surf, corner, outlier)
 *               and VoxelGrid(lc_leaf)-filtered; ICP and fitness exactly as alego_loop_search runs them.  Accepted when converged &&
 *               fitness <= lc_fitness_max; the first accepted candidate ends the slot.  t_map = correction * matrix(guess6), as t_correct of
 *               alego_loop_constraint.
 *   apply       accepted slots with apply = 1: rc = t_map * T_cur^-1 in f64 (T_cur = the slot's t_map2laser_ of its last mapping frame,
 *               R_rc = R_map R_cur^T, c = t_map - R_rc t_cur), params6 = (translation of t_map, roll = atan2(R21, R22), pitch = atan2(-R20,
 *               sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00) of its rotation); map -> odom and params_ are set as alego_lm_apply_correction(rc)
 *               and alego_set_lm_params(params6) set them.  The window is left alone: the next mapping frame selects at the new pose.
 * alego_reloc_enable     once, after alego_loc_enable (else ALEGO_ERR_ARG; a second call too): builds the N map descriptors and ring keys on the
 *                        device.  max_range <= 0: 80.0; z_offset not finite: 4.0.  Device memory: 1240 B per frame of the store's capacity and per slot; search and
 *                        ICP scratch grows on first use and stays with the handle.  Without the call nothing is allocated or launched.
 * alego_loc_relocalize   synchronous; runs behind the work queued on every stream group.  out[i] belongs to slots[i]; a slot's result does not
 *                        depend on the other slots, their order or the chunking.  ALEGO_ERR_ARG: not enabled, a slot out of range or listed
 *                        twice, n_cand > ALEGO_RELOC_MAX_CAND, verify > n_cand.  opts == NULL: n_cand 4, verify 1, apply 0; n_cand <= 0: 4;
 *                        verify < 0: 1; verify == 0: search only.
 * alego_reloc_descriptor / alego_reloc_match   host only, plain C++: the rule on one cloud / one pair of descriptors.
 * alego_debug_reloc_search   the search kernels alone on descriptors the caller supplies (tests): ids / dists / shifts [n_q][n_cand], -1 where
 *                        n_map < n_cand.  alego_debug_set_option("ALEGO_RL_BRUTE", 1) evaluates every (query, frame) pair instead of pruning
 *                        with the ring-key bound; "ALEGO_RL_BUDGET" sets the (query, frame) pairs per chunk of the search.  These three debug
 *                        entries work on any handle and are the one exception to "nothing is allocated without alego_reloc_enable": the
 *                        first of them creates the search context (and, for the search, its scratch), which the handle then keeps;
 *                        alego_debug_get("rl_stats") (pairs the second round evaluated, pairs in all, of the last search) answers there too.
 * alego_debug_get names: "rl_query_desc" (the slot's 1200 bytes), "rl_query_key" (40 bytes: 20 u16), "rl_map_desc", "rl_map_key" (all N frames). */
#define ALEGO_RELOC_MAX_CAND 8
typedef struct alego_reloc_opts {
  int32_t n_cand;          /* 1 .. ALEGO_RELOC_MAX_CAND */
  int32_t verify;          /* candidates verified at most, 0 .. n_cand */
  int32_t apply;           /* 1: place every accepted slot on the device */
} alego_reloc_opts;
typedef struct alego_reloc_result {
  int32_t status;          /* 2 accepted; 1 candidates but none accepted (or verify == 0); 0 no mapping frame yet, no point in range or an empty map */
  int32_t n_cand;
  int32_t cand_id[ALEGO_RELOC_MAX_CAND], cand_dist[ALEGO_RELOC_MAX_CAND], cand_shift[ALEGO_RELOC_MAX_CAND];
  int32_t verified;        /* index into the candidates of the accepted one, or -1 */
  int32_t converged, iterations, n_source, n_target;   /* of the last candidate verified */
  int32_t applied;
  double fitness;
  float correction[16];    /* getFinalTransformation(), row-major */
  float guess6[6];         /* the ICP's initial guess (the last candidate verified) */
  float t_map[16];         /* correction * matrix(guess6): the sensor pose in the map */
  double rc[12];           /* row-major 3x4 for alego_lm_apply_correction (accepted slots) */
  double params6[6];       /* for alego_set_lm_params (accepted slots) */
} alego_reloc_result;
int alego_reloc_enable(alego_handle* h, double max_range, double z_offset);
int alego_loc_relocalize(alego_handle* h, const int32_t* slots, int32_t n, const alego_reloc_opts* opts, alego_reloc_result* out);
int alego_reloc_descriptor(const alego_point* pts, int32_t n, double max_range, double z_offset, uint8_t* desc1200, uint16_t* key20);
int alego_reloc_match(const uint8_t* q1200, const uint8_t* m1200, int32_t* dist, int32_t* shift);
int alego_debug_reloc_search(alego_handle* h, const uint8_t* map_desc, int32_t n_map, const uint8_t* q_desc, int32_t n_q, int32_t n_cand,
                             int32_t* ids, int32_t* dists, int32_t* shifts);

/* ---- loop closures by appearance: a SLAM slot searched against its OWN archive (needs alego_map_enable) -----
 * alego_loop_search finds a revisit only while the accumulated drift is smaller than lc_search_radius.  This search recognises the place from
 * the clouds instead, with the descriptor, the exact pruned search and the yaw-shifted guess of relocalisation (above) and the ICP of
 * alego_loop_search.  The rule (the project's own; csrc/kernels_reloc.hip states it next to the kernels), for a listed slot with nf archived
 * frames and none dropped:
 *   query       the descriptor of the newest archived frame nf - 1 (its corner, surf and outlier clouds)
 *   eligible    frame i < nf - 1 with stamp[nf - 1] - stamp[i] > lc_min_time_gap and, when max_jump > 0, the f32 squared distance
 *               ((dx dx) + dy dy) + dz dz of key poses i and nf - 1 < (float)(max_jump * max_jump).  A predicate per frame, not a prefix.
 *   candidates  the n_cand eligible frames smallest in (D_i, i), D_i and s_i as alego_reloc_match: exactly the brute force over all eligible
 *               frames and all 60 shifts; candidates with D_i > max_dist are dropped when max_dist > 0
 *   verify      candidate v in round v, at most `verify` rounds, the first accepted ends the slot: source = frame nf - 1 (surf, corner, outlier)
 *               under guess6 = key pose i with yaw - (float)s_i * (float)(2 pi / 60); target = frames [i - lc_search_num, i + lc_search_num]
 *               within [0, nf - 2] under their archived poses through VoxelGrid(lc_leaf); ICP and fitness exactly as alego_loop_search runs
 *               them.  Accepted when converged && fitness <= fitness_max (fitness_max <= 0: lc_fitness_max).
 *   result      an alego_loop_result that alego_graph_add_loops takes unchanged: latest_id = nf - 1; closest_id = the accepted candidate, or
 *               the last one verified, or the first candidate when verify == 0, or -1; t_correct and between = alego_loop_constraint(the ICP's
 *               final transformation, guess6, key pose closest_id); noise_variance = (float)fitness; correction = the WORLD correction
 *               t_correct * matrix(key pose nf - 1)^-1 (f32 matrices widened to f64, rigid inverse, product rounded to f32) - with guess6 equal
 *               to the newest key pose that is the ICP's final transformation, which alego_loop_search stores there, and it is what apply = 1 of
 *               alego_graph_optimize hands to map -> odom.  status: 0 no key frame, no eligible frame, an empty query descriptor or no
 *               candidate left after max_dist; 1 attempted and rejected, or verify == 0; 2 accepted; -1 the archive dropped frames.
 * alego_loop_appearance_enable   once, any time after alego_map_enable (ALEGO_ERR_ARG: a second call, without the archive, on a localising
 *                        handle).  max_range <= 0: 80.0; z_offset not finite: 4.0.  Device memory: max_keyframes * 1240 B + 732 B per slot.
 *                        Descriptors are built lazily: a search first describes the listed slots' frames [described, nf) (archived clouds never
 *                        change once stored); nothing is added to the per-scan path.  Without the call nothing is allocated or launched.
 * alego_loop_search_appearance   synchronous; runs behind the work queued on every stream group and changes no device state.  out[i] (and
 *                        info[i], when info is not NULL) belongs to slots[i]; a slot's result does not depend on the other slots, their order or
 *                        the chunking.  opts == NULL: n_cand 4, verify 1, gates off; n_cand <= 0: 4; verify < 0: 1; verify == 0: search only.
 *                        ALEGO_ERR_ARG: not enabled, a slot out of range or listed twice, n_cand > ALEGO_RELOC_MAX_CAND, verify > n_cand.
 * alego_loop_appearance_candidates   host only, plain C++: the candidates of frame n - 1 of desc[n][1200] over frames 0 .. n - 2; returns their
 *                        count (ids / dists / shifts hold n_cand entries each), 0 for n < 2 or an all-zero descriptor of frame n - 1.
 * alego_debug_get names: "la_desc" ([frames described][1200] bytes of the slot), "la_key" ([frames described] x 20 u16).  "ALEGO_RL_BRUTE" and
 * "ALEGO_RL_BUDGET" act on this search as on relocalisation's. */
typedef struct alego_loop_app_opts {
  int32_t n_cand, verify, max_dist;
  double max_jump, fitness_max;
} alego_loop_app_opts;
typedef struct alego_loop_app_info {
  int32_t n_eligible, n_cand;   /* eligible frames; candidates left after max_dist */
  int32_t cand_id[ALEGO_RELOC_MAX_CAND], cand_dist[ALEGO_RELOC_MAX_CAND], cand_shift[ALEGO_RELOC_MAX_CAND];
  int32_t verified;             /* index of the accepted candidate or -1 */
  float guess6[6];              /* the ICP's initial guess (the last candidate verified) */
  float icp_final[16];          /* its getFinalTransformation(), row-major */
} alego_loop_app_info;
int alego_loop_appearance_enable(alego_handle* h, double max_range, double z_offset);
int alego_loop_search_appearance(alego_handle* h, const int32_t* slots, int32_t n, const alego_loop_app_opts* opts, alego_loop_result* out,
                                 alego_loop_app_info* info);
int alego_loop_appearance_candidates(const uint8_t* desc, const float* keyposes6, const double* stamps, int32_t n, double min_time_gap,
                                     double max_jump, int32_t max_dist, int32_t n_cand, int32_t* ids, int32_t* dists, int32_t* shifts);

/* ---- aligning one slot's key-frame archive to another's by appearance (needs alego_loop_appearance_enable) -------
 * Every archive sits in the frame of its own first scan.  alego_map_align asks, for pairs (src, dst) of slots, which rigid transform takes the
 * source archive into the destination's frame: several source frames are searched in the destination's descriptors and verified by the ICP
 * of alego_loop_search, and the answers of the queries decide among themselves - true answers agree on one transform, aliased ones do not.
 * The rule (the project's own; csrc/align_math.h and csrc/kernels_reloc.hip state it next to the code), for a pair with ns source and nd
 * destination frames archived and none dropped:
 *   queries     Q = min(n_queries, ns); query q is source frame ((2 q + 1) ns) / (2 Q) in integer arithmetic, the middle of the q-th of Q equal
 *               stretches: distinct and ascending.  alego_map_align_queries is the same function.
 *   search      every query over ALL nd destination frames, no eligibility predicate: the n_cand frames smallest in (D_i, i), D_i and s_i as
 *               alego_reloc_match - exactly the brute force over all frames and all 60 shifts; candidates with D_i > max_dist are dropped when
 *               max_dist > 0; a query whose ring key is all zero (no point in range) has none.
 *   verify      per query, candidates in order, the first accepted ends the query: source = source frame f (surf, corner, outlier) under
 *               guess6 = destination key pose i with yaw - (float)s_i * (float)(2 pi / 60); target = destination frames [i - lc_search_num,
 *               i + lc_search_num] within [0, nd - 1] under their archived poses through VoxelGrid(lc_leaf); ICP and fitness exactly as
 *               alego_loop_search runs them.  Accepted when converged && fitness <= fitness_max (fitness_max <= 0: lc_fitness_max).
 *   hypothesis  T = t_correct * matrix(source key pose f)^-1, t_correct = icp_final * matrix(guess6) as alego_loop_constraint builds it; f32
 *               matrices widened to f64, the rigid inverse, the product rounded to f32 - the arithmetic of the appearance search's correction.
 *   consensus   accepted hypotheses a and b AGREE when the angle of R_a^T R_b, taken as atan2(|v|, c) with v = vee(M - M^T) / 2 and
 *               c = (tr M - 1) / 2, is <= tol_rot and, at both query positions p_a and p_b (the source key-pose xyz), |T_a p - T_b p| <=
 *               tol_trans; f64 without contraction.  Positions are compared rather than the translation columns, so that a small rotation error
 *               far from the origin counts.  A non-finite T agrees with nothing, itself included.  support(a) = the accepted b that agree with a,
 *               a included; best = the largest support (>= 1), ties to the smaller own fitness, then to the smaller index; inlier marks the
 *               hypotheses that agree with the best one.  The result's T is the best hypothesis itself: no averaging.
 *   status      -1 an archive of the pair dropped frames; 0 nothing to try (an empty archive, or no query had a candidate); 2 when
 *               support(best) >= min_support; 1 otherwise.
 * Defaults of tol_trans / tol_rot, measured on the reference-side emulation of tests/test_map_align.py (two oracle-mapped stretches of the
 * synthetic lap; DESIGN.md section 17 has the tables): A = the largest pairwise disagreement among hypotheses within 0.25 m / 0.02 rad of the
 * ground truth, B = the smallest disagreement between such a hypothesis and one that is not; the defaults are 2 A and must stay below B / 2.
 *   A = 0.1197 m / 0.00825 rad, B = 29.27 m / 3.1385 rad (an aliased place lies half a turn away), so
 *   ALEGO_ALIGN_TOL_TRANS   0.24 m       (2 A rounded up; B / 2 = 14.6 m)
 *   ALEGO_ALIGN_TOL_ROT     0.0165 rad   (2 A rounded up; B / 2 = 1.57 rad)
 * alego_map_align         synchronous; runs behind the work queued on every stream group and changes no device state.  out[i] (and
 *                         hyp[i][0 .. ALEGO_ALIGN_MAX_QUERIES), when hyp is not NULL) belongs to the pair (src_slots[i], dst_slots[i]); a pair's
 *                         result does not depend on the other pairs, their order or the chunking, and a slot may appear in many pairs.
 *                         opts == NULL or a field <= 0: n_queries 8, n_cand 2, max_dist off, min_support 2, fitness_max lc_fitness_max, the
 *                         tolerances above.  ALEGO_ERR_ARG: a localising handle, the appearance search not enabled, a slot out
 *                         of range, src == dst in a pair, a pair listed twice, n_queries > ALEGO_ALIGN_MAX_QUERIES, n_cand > ALEGO_RELOC_MAX_CAND.
 *                         Descriptors of both archives are built lazily as by alego_loop_search_appearance; scratch grows with the calls and
 *                         stays with the handle.  Without a call nothing is allocated or launched.
 * alego_map_align_queries   host only, plain C++: the query frames of an archive of n_frames; returns Q (n_queries <= 0: 8).
 * alego_map_align_consensus host only, plain C++: support[n] and *best (-1: none) of n <= ALEGO_ALIGN_MAX_QUERIES hypotheses T16[n][16] (row-major
 *                         4 x 4, rows 0 .. 2 read) with query positions src_pos3[n][3] - the arithmetic the kernel runs.  tol <= 0: the defaults.
 *                         The sums, products and the square root are the same f64 on both sides; atan2 comes from two libraries (the device's and
 *                         the host's), so a pair whose angle lies within an ulp of tol_rot may be judged differently by the two.
 * alego_map_align_poses   host only, plain C++: out6[i] = the f32 key pose of T12 * Pose3(RzRyRx(roll, pitch, yaw), xyz) of poses6[i], f64, back
 *                         to (x y z, roll = atan2(R21, R22), pitch = atan2(-R20, sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00)) as alego_graph_optimize
 *                         writes poses.  The caller moves an archive with the calls that exist: alego_map_set_keyposes, alego_lm_set_keypose,
 *                         alego_lm_reset_window, alego_lm_apply_correction - or, for whole slots on the device, with alego_map_move (below). */
#define ALEGO_ALIGN_MAX_QUERIES 32
#define ALEGO_ALIGN_TOL_TRANS 0.24    /* m */
#define ALEGO_ALIGN_TOL_ROT 0.0165    /* rad */
typedef struct alego_map_align_opts {
  int32_t n_queries;       /* 1 .. ALEGO_ALIGN_MAX_QUERIES; <= 0: 8 */
  int32_t n_cand;          /* candidates per query, 1 .. ALEGO_RELOC_MAX_CAND; <= 0: 2 */
  int32_t max_dist;        /* > 0: candidates with D above it are dropped */
  int32_t min_support;     /* <= 0: 2 */
  double fitness_max;      /* <= 0: lc_fitness_max */
  double tol_trans, tol_rot;   /* agreement of two hypotheses, m / rad; <= 0: ALEGO_ALIGN_TOL_TRANS / ALEGO_ALIGN_TOL_ROT */
} alego_map_align_opts;
typedef struct alego_map_align_hyp {   /* one per query */
  int32_t src_frame, dst_frame, dist, shift;   /* the last candidate verified (the accepted one when accepted); dst_frame -1: the query had no candidate */
  int32_t tried, accepted;                     /* candidates verified; 1 when one was accepted */
  int32_t converged, iterations, n_source, n_target;
  int32_t support, inlier;                     /* accepted hypotheses agreeing with this one (itself included); 1 when it agrees with the best */
  double fitness;
  float guess6[6], icp_final[16];
  float T[16];                                 /* dst <- src of this hypothesis, row-major */
} alego_map_align_hyp;
typedef struct alego_map_align_result {
  int32_t status;          /* 2 aligned; 1 hypotheses but support < min_support; 0 nothing to try; -1 an archive of the pair dropped frames */
  int32_t n_queries, n_accepted, best, support;   /* best: index of the chosen hypothesis or -1 */
  double T[12];            /* dst <- src, row-major 3x4: the chosen hypothesis' T widened to f64 */
} alego_map_align_result;
int alego_map_align(alego_handle* h, const int32_t* src_slots, const int32_t* dst_slots, int32_t n, const alego_map_align_opts* opts,
                    alego_map_align_result* out, alego_map_align_hyp* hyp /* NULL or [n][ALEGO_ALIGN_MAX_QUERIES] */);
int alego_map_align_queries(int32_t n_frames, int32_t n_queries, int32_t* frames);
int alego_map_align_consensus(const float* T16, const float* src_pos3, const double* fitness, const int32_t* accepted, int32_t n,
                              double tol_trans, double tol_rot, int32_t* support, int32_t* best);
int alego_map_align_poses(const double T12[12], const float* poses6, int32_t n, float* out6);

/* ---- moving a slot and merging one slot's archive into another's, on the device (needs alego_map_enable) ----------
 * alego_map_align says which rigid transform takes one archive into the frame of another; these two calls act on it without a frame leaving
 * the device.  Both are synchronous, run behind the work queued on every stream group, are refused (ALEGO_ERR_ARG) on a localising handle and
 * with the archive off; their graph parts apply only after alego_graph_enable.  Without a call nothing is allocated or launched.  Each call is
 * DEFINED by a sequence of the calls above and leaves the device state that sequence leaves, as every getter and every later scan sees it.
 * The pose arithmetic is alego_map_align_poses' (csrc/merge_math.h); its sin, cos and atan2 come from the device's library here and from the
 * host's there, so a pose component may differ from alego_map_align_poses in its last f32 bit; everything else is exact.
 *
 * alego_map_move   applies the row-major 3x4 T12[i] to the whole slot slots[i] of N archived frames; the state of
 *     alego_map_set_keyposes(s, 0, N, alego_map_align_poses(T, archived poses)); alego_lm_set_keypose with the same pose for every resident frame,
 *     oldest first; alego_lm_reset_window; alego_lm_apply_correction(s, T); and, with the graph on, chain edge 0 (the prior) rewritten to
 *     between <- T * between as alego_graph_set_edges writes it (without that the next alego_graph_optimize pulls the slot back).  No other edge
 *     changes, and neither does the last estimate.  out_status[i]: 2 moved, 0 no key frame, -1 the archive dropped frames (nothing written).
 *     ALEGO_ERR_ARG: a slot out of range or listed twice, a non-finite T; nothing is written then.
 * alego_map_merge  appends, for every pair, the source archive moved by T12[i] behind the destination's; the source slot is not changed.  With
 *     ns source and nd destination frames the state of dst is that of
 *       alego_lm_reset_window(dst);
 *       alego_lm_add_keyframe(dst, moved pose of f, clouds of source frame f as archived) for f = 0 .. ns - 1;
 *       alego_map_set_stamps(dst, nd, ns, source stamps + opts.stamp_offset) (one f64 add);
 *     and, with the graph on,
 *       chain edges nd + 1 .. nd + ns - 1 overwritten by the source's chain edges 1 .. ns - 1 with both ids raised by nd (a measurement stays
 *       what was measured; it is not recomputed from the poses);
 *       chain edge nd, the SEAM, as the archive recorded it - between(pose nd - 1 as archived now, the first moved pose), or the prior when
 *       nd == 0 - with the variances opts.seam_variance.  NULL there means the graph's odometry variance, which asserts T with odometry
 *       certainty: a caller who passes hypotheses wants the cross edges to decide and must pass a LOOSE seam;
 *       the source's loop edges in their order, ids raised by nd, as alego_graph_add_edge(dst, e, NULL) appends them;
 *       with hyp != NULL (the pair's [ALEGO_ALIGN_MAX_QUERIES] hypotheses of alego_map_align; entries beyond the pair's queries zero), for every
 *       hypothesis with accepted && inlier, in index order, the edge of alego_map_align_edge, appended the same way.
 *     The last estimate of dst stays what it was.  Descriptors of the appended frames are built lazily by the next appearance search or alignment.
 *     out[i].status: 2 merged; 0 empty source; -1 an archive of the pair dropped frames; -3 does not fit (nd + ns > max_keyframes, points over
 *     max_points, or destination loops + source loops + inlier edges over max_loops).  For every status but 2 dst is byte-unchanged, and the
 *     other pairs proceed: all counts are known after the initial synchronisation, so every check happens before anything is written.
 *     ALEGO_ERR_ARG (nothing written): a slot out of range, src == dst, a destination listed twice, a slot that is a destination of one pair
 *     and a source of another, a non-finite T, a seam_variance that is not positive and finite, a non-finite stamp_offset, an inlier
 *     hypothesis whose frames lie outside the archives or whose edge alego_graph_add_edge would refuse.  A source may feed many destinations.
 * alego_map_align_edge   host only, plain C++: the cross edge of one hypothesis for a destination of nd frames: from = nd + src_frame,
 *     to = dst_frame, between = that of alego_loop_constraint(icp_final, guess6, dst_pose6) with dst_pose6 the destination's key pose of
 *     dst_frame, all six variances (float)fitness as alego_graph_add_loops sets them.  ALEGO_ERR_ARG unless accepted && inlier.
 * alego_map_merge_edges  host only, plain C++ over csrc/merge_math.h (the arithmetic the kernel runs): the graph part of a merge from plain
 *     arrays.  out_chain[ns]: [0] the seam (prev_pose6 = destination key pose nd - 1, unused for nd == 0; first_pose6 = the first moved pose;
 *     seam_variance6), [f] = src_chain[f] shifted by nd; out_loops[n_loops] = src_loops shifted by nd.
 * Out of scope: continuing the SOURCE's live stream inside the union (its LaserOdometry / LaserMapping state would have to move as well).
 * Duplicate frames of the overlap are removed by alego_map_thin (below). */
#define ALEGO_MERGE_COPY_ITEM 1024   /* points per work item of the archive-to-archive copy: one workgroup copies this many at 16 B per lane and access */
typedef struct alego_map_merge_opts {
  double stamp_offset;           /* added to every source stamp */
  const double* seam_variance;   /* [6] rotation x y z, translation x y z of chain edge nd; NULL: the graph's odometry variance */
} alego_map_merge_opts;
typedef struct alego_map_merge_result {
  int32_t status;                /* 2 merged, 0 empty source, -1 an archive of the pair dropped frames, -3 does not fit */
  int32_t frames, points;        /* appended to dst */
  int32_t loop_edges, cross_edges;   /* the source's loop edges / the hypotheses' edges appended to dst */
} alego_map_merge_result;
int alego_map_move(alego_handle* h, const int32_t* slots, int32_t n, const double* T12 /* [n][12] */, int32_t* out_status);
int alego_map_merge(alego_handle* h, const int32_t* src_slots, const int32_t* dst_slots, int32_t n, const double* T12 /* [n][12] */,
                    const alego_map_merge_opts* opts, const alego_map_align_hyp* hyp /* NULL or [n][ALEGO_ALIGN_MAX_QUERIES] */, alego_map_merge_result* out);
int alego_map_align_edge(const alego_map_align_hyp* hyp, const float dst_pose6[6], int32_t nd, alego_graph_edge* edge);
int alego_map_merge_edges(const alego_graph_edge* src_chain, int32_t ns, const alego_graph_edge* src_loops, int32_t n_loops, int32_t nd,
                          const float prev_pose6[6], const float first_pose6[6], const double seam_variance6[6],
                          alego_graph_edge* out_chain, alego_graph_edge* out_loops);

/* ---- thinning a slot's key-frame archive on the device (needs alego_map_enable) ----------------------------------
 * A merged archive covers the overlap twice, a long session the same road N times, and an archive that reached max_keyframes or max_points
 * drops every later frame.  alego_map_thin removes frames that lie closer than min_dist to a frame that stays, in place, for many slots per
 * call, and gives the room back.  Synchronous; runs behind the work queued on every stream group; its graph part applies only after
 * alego_graph_enable.  Without a call nothing is allocated or launched.  The rule (the project's own; csrc/thin_math.h states it next to the
 * code), for a listed slot with N archived frames and none dropped:
 *   protected   frame 0; the newest min(N, recent_keyframe_num + 1) frames (the resident ring); both endpoints of every stored loop edge.
 *               A protected frame is always kept.
 *   selection   frames are visited in id order; an unprotected frame i is DROPPED iff some KEPT frame j < i has the f32 squared distance of
 *               the key-pose positions ((dx dx) + dy dy) + dz dz < (float)(min_dist * min_dist) - the comparison of alego_loc_select.  Greedy: a
 *               dropped frame suppresses nobody.  A non-finite position makes every comparison false (kept, suppresses nothing); min_dist <= 0
 *               drops nothing.  Position only, so device and host agree bit for bit.
 *   archive     the kept frames k_0 = 0 < k_1 < ... keep pose, stamp and clouds and become frames 0 .. N' - 1; their points are one contiguous
 *               prefix in id order; alego_map_status says {N', 0, P'}.
 *   chain       new chain edge m (m - 1 -> m): the f64 product of the old chain measurements k_(m-1) + 1 .. k_m in that order, associated left to
 *               right; its six variances are the component-wise sums of the composed edges' variances - a FIRST-ORDER rule that ignores how the
 *               intermediate rotations mix the components.  A measurement stays what was measured: nothing is recomputed from poses.  Edge 0,
 *               the prior, is unchanged.
 *   loops       every loop edge keeps measurement and variances; its ids are renumbered (its endpoints are protected, so they exist).
 *               loop_closed_ stays as it was; the last estimate is discarded (alego_graph_status out[3] becomes 0).
 *   live slot   alego_lm_keyframe_count becomes N'; the window is reset as by alego_lm_reset_window; the ring holds the newest min(N', K + 1)
 *               frames under their NEW ids, re-transformed and sorted oldest first - the state of alego_lm_reset_window followed by
 *               alego_lm_add_keyframe of every kept frame in a fresh slot.  map -> odom, params_, the LaserOdometry state and the trajectory
 *               are untouched: the stream continues, its next key frame gets id N' and a chain edge from frame N' - 1.
 *   descriptors the appearance descriptors stay valid below the first dropped frame; the rest is described again lazily.
 * out[i].status: 2 thinned (frames_before, frames, points_before, points filled); 1 nothing to drop - the slot is byte-unchanged and its
 * window is not reset; 0 no key frame; -1 the archive dropped frames, untouched.  A slot's result does not depend on the other slots of the
 * call or their order.  opts == NULL: min_dist 0.  ALEGO_ERR_ARG (nothing written): a localising handle, the archive off, a slot out of range
 * or listed twice, a min_dist that is not finite.
 * alego_map_thin_select   host only, plain C++ over csrc/thin_math.h (the arithmetic the kernel runs): keep[n] (1 kept, 0 dropped) for
 *     keyposes6[n][6] and the protect byte mask (NULL: no frame protected); returns the frames kept.
 * alego_map_thin_edges    host only: out_chain[N'] and out_loops[n_loops] from a chain of n edges (edge 0 the prior), loop edges and a keep mask
 *     with keep[0] set; returns N'.  ALEGO_ERR_ARG when an endpoint of a loop edge is dropped or out of range.
 * alego_debug_thin_select runs the selection kernel alone on arrays of the caller (protect required); returns the frames kept. */
typedef struct alego_map_thin_opts {
  double min_dist;               /* m; <= 0: nothing is dropped */
} alego_map_thin_opts;
typedef struct alego_map_thin_result {
  int32_t status;                /* 2 thinned, 1 nothing to drop, 0 no key frame, -1 the archive dropped frames */
  int32_t frames_before, frames, points_before, points;
} alego_map_thin_result;
int alego_map_thin(alego_handle* h, const int32_t* slots, int32_t n, const alego_map_thin_opts* opts, alego_map_thin_result* out);
int alego_map_thin_select(const float* keyposes6, const uint8_t* protect, int32_t n, double min_dist, uint8_t* keep);
int alego_map_thin_edges(const alego_graph_edge* chain, int32_t n, const alego_graph_edge* loops, int32_t n_loops, const uint8_t* keep,
                         alego_graph_edge* out_chain, alego_graph_edge* out_loops);
int alego_debug_thin_select(alego_handle* h, const float* keyposes6, const uint8_t* protect, int32_t n, double min_dist, uint8_t* keep);

/* ---- occupancy grid of the key-frame archive by ray casting (csrc/kernels_occ.hip, csrc/occ_math.h) ------------
 * Not part of the reference.  Every archived point is a ray from its frame's key-pose position to a surface: the cells a ray passes
 * were seen free, the cell it ends in holds something, a cell no ray visits was never observed.  Opt-in: without alego_occ_enable
 * nothing is allocated or launched, and nothing on the per-scan path changes.
 *
 * GRID    origin[3] = world position of the corner of cell (0, 0, 0); cell[3] > 0 the edge lengths; n[3] >= 1 cells per axis with
 *         n[0] n[1] n[2] <= 2^31 - 1; linear index (z n[1] + y) n[0] + x.  One thick layer (n[2] = 1) is the 2-D product.
 * RAY     from the key pose's translation to the point as alego_map_assemble gives it (f32), widened to f64.  A ray with a non-finite
 *         coordinate or an end further than 2^30 cells from the origin is BAD; one shorter than min_range is SHORT; one longer than
 *         max_range (> 0; 0: no limit) is TRUNCATED to that length and carries no hit; one whose end cells lie on the same outer side of
 *         the grid on some axis is CULLED.  Bad, short and culled rays change nothing.  The cells between are those of an exact
 *         voxel traversal with ties to the lowest axis (csrc/occ_math.h states the rule; the kernel and the host twins share it).
 * COUNTS  u32 per cell: every visited cell but the last passes += 1; the last hits += 1, or passes += 1 for a truncated ray.  Integer
 *         adds: the result does not depend on the order of arrival, device and host agree exactly.  There is no per-scan de-duplication.
 * CLASSES 100 (occupied) iff hits >= min_hits and hits * hit_weight >= passes * pass_weight (64-bit); else 0 (free) if passes > 0; else
 *         -1 (unknown).  The defaults 1, 2, 1 (rule = NULL) are parameters of a model, not measurements.  collapse_z = 1 writes one
 *         value per (x, y) column (100 if any layer is 100, else 0 if any is 0, else -1): the layout of a nav_msgs/OccupancyGrid.
 *
 * alego_occ_enable     once per mapping handle with the archive on: allocates and zeroes the grid.
 * alego_occ_clear      zeroes the counts.
 * alego_occ_integrate  adds the rays of frames [first, first + n) (n = -1: to the newest) of `slot`, clouds `kinds`
 *                      (ALEGO_MAP_SURF | _CORNER | _OUTLIER), at the poses that hold NOW; synchronous, behind the slot's own stream.  It
 *                      accumulates: several calls or slots add up.  stats (may be NULL) gets this call's counters.
 * alego_occ_get        the counts, n[0] n[1] n[2] each (either pointer may be NULL).
 * alego_occ_classify   out[cells], or out[n[0] n[1]] with collapse_z.
 * Every refusal is ALEGO_ERR_ARG with alego_last_error set: archive off, a second enable, a call before enable, options out of range,
 * frames beyond those stored, kinds without a cloud, a slot out of range, a negative weight or min_hits.
 * Host twins (no device, no handle): alego_occ_ray_host writes the first `cap` visited cells of one ray to cells3[3 i + k] and returns how
 * many the ray visits or ALEGO_OCC_SKIP_*; *hit = 1 when the last cell takes a hit.  alego_occ_integrate_host adds points (w = frame id, as
 * alego_map_assemble gives them with ALEGO_MAP_FRAME_ID) cast from origins[frame] (alego_map_keyposes) into hits / passes / stats, which it
 * does NOT zero (a negative or NaN frame id: ALEGO_ERR_ARG, nothing added; an id beyond the origins is the caller's to avoid).  alego_occ_classify_host is
 * alego_occ_classify on host arrays. */
typedef struct alego_occ_opts { double origin[3], cell[3]; int32_t n[3], pad; double min_range, max_range; } alego_occ_opts;
typedef struct alego_occ_rule { int32_t min_hits, hit_weight, pass_weight, pad; } alego_occ_rule;
/* counters of one integrate (int64 each): rays read, of them short / truncated / culled / bad, cell updates inside the grid */
enum { ALEGO_OCC_RAYS = 0, ALEGO_OCC_SHORT, ALEGO_OCC_TRUNCATED, ALEGO_OCC_CULLED, ALEGO_OCC_BAD, ALEGO_OCC_UPDATES, ALEGO_OCC_STATS };
enum { ALEGO_OCC_SKIP_SHORT = -10, ALEGO_OCC_SKIP_CULLED = -11, ALEGO_OCC_SKIP_BAD = -12 };
int alego_occ_enable(alego_handle* h, const alego_occ_opts* opts);
int alego_occ_clear(alego_handle* h);
int alego_occ_integrate(alego_handle* h, int slot, int32_t first, int32_t n, int kinds, int64_t stats[ALEGO_OCC_STATS]);
int alego_occ_get(alego_handle* h, uint32_t* hits, uint32_t* passes);
int alego_occ_classify(alego_handle* h, const alego_occ_rule* rule, int collapse_z, int8_t* out);
int alego_occ_ray_host(const alego_occ_opts* opts, const float o[3], const float e[3], int32_t* cells3, int32_t cap, int32_t* hit);
int alego_occ_integrate_host(const alego_occ_opts* opts, const alego_point* origins, const alego_point* pts, int32_t n_pts, uint32_t* hits, uint32_t* passes,
                             int64_t stats[ALEGO_OCC_STATS]);
int alego_occ_classify_host(const alego_occ_opts* opts, const alego_occ_rule* rule, const uint32_t* hits, const uint32_t* passes, int collapse_z, int8_t* out);
/* development: the piece length of occ_cast's work distribution for this handle (steps of a ray one lane walks at a time; <= 0: one lane
 * walks a whole ray, the baseline tools/occ_timing.py measures next to the default).  The counts do not depend on it. */
int alego_debug_occ_piece(alego_handle* h, int32_t piece);

/* ---- clearance field and inflated cost map of the occupancy grid (csrc/kernels_edt.hip, csrc/edt_math.h) ---------
 * Not part of the reference.  What a planner reads off the grid is how far every cell is from the nearest obstacle: the clearance of a
 * path, costmap_2d's inflation layer, an ESDF.  The exact squared Euclidean distance transform of the classified grid, in integers: device
 * and host agree exactly.  Nothing is allocated or launched without these calls; the counts are not changed.
 *
 * DOMAIN   the class array alego_occ_classify gives: n[0] n[1] n[2] cells, or n[0] n[1] with collapse_z.  An axis with one cell contributes
 *          no displacement; every axis with more than one cell must have the same edge length s (compared as doubles; no such axis:
 *          s = cell[0]), and the sum of (n_k - 1)^2 over the axes must not exceed 2^32 - 2, so that no finite value reaches FAR.
 * SOURCES  the cells of class 100; with unknown_is_obstacle those of class -1 as well.
 * D2       u32 per cell: the minimum over the sources of dx^2 + dy^2 + dz^2 in cells; ALEGO_OCC_FAR where there is no source.
 *          max_cells = r > 0 turns every d2 > r^2 into FAR; 0: no limit; r < 0 or r > 65535 is refused.  The distance is s sqrt(d2).
 * TABLE    costmap_2d's computeCost over d2: r = ceil(inflation_radius / s); table[0] = 254; for 1 <= d2 <= r^2 with
 *          dist = sqrt((double) d2) s: 253 if dist <= inscribed_radius, else (uint8_t)(252.0 exp(-cost_scaling (dist - inscribed_radius))).
 *          Refused: a non-finite or negative radius or scaling, inflation_radius < inscribed_radius, r > 4095.
 * COST     254 on a source; else t = table[d2] (0 beyond the table or where d2 is FAR): a free cell gets t, an unknown one t if
 *          t >= (inflate_unknown ? 1 : 253), else 255 (NO_INFORMATION).
 *
 * alego_occ_set       the counterpart of alego_occ_get: copies counts to the grid (either pointer may be NULL: that array keeps its counts).
 * alego_occ_distance  classifies on the device under `rule` (NULL: the defaults), transforms, and copies d2 (may be NULL: stats only) and
 *                     stats (may be NULL) out; opts = NULL: {0, 0, 0, 0}.  stats: sources, FAR cells, the largest finite d2 (-1: none).
 * alego_occ_costmap   the same with max_cells = r, then the cost of every cell to out.
 * Both are synchronous and need a mapping handle with the archive on and the grid enabled.  Every refusal is ALEGO_ERR_ARG with
 * alego_last_error set.
 * Host twins (no device, no handle): alego_occ_distance_host takes what alego_occ_classify / alego_occ_classify_host gave (for a collapsed
 * grid pass n[2] = 1); d2 or stats may be NULL.  alego_occ_cost_table_host writes table[0, r r] and returns r r + 1 (cap below that:
 * ALEGO_ERR_CAPACITY).  alego_occ_costmap_host is the cost rule over `cells` cells. */
#define ALEGO_OCC_FAR 0xFFFFFFFFu
typedef struct alego_occ_dist_opts { int32_t collapse_z, unknown_is_obstacle, max_cells, pad; } alego_occ_dist_opts;
typedef struct alego_occ_inflation { double inscribed_radius, inflation_radius, cost_scaling; int32_t inflate_unknown, pad; } alego_occ_inflation;
/* int64 each: sources, FAR cells, the largest finite d2 (-1: none) */
enum { ALEGO_EDT_SOURCES = 0, ALEGO_EDT_FAR_CELLS, ALEGO_EDT_MAX_D2, ALEGO_EDT_STATS };
int alego_occ_set(alego_handle* h, const uint32_t* hits, const uint32_t* passes);
int alego_occ_distance(alego_handle* h, const alego_occ_rule* rule, const alego_occ_dist_opts* opts, uint32_t* d2, int64_t stats[ALEGO_EDT_STATS]);
int alego_occ_costmap(alego_handle* h, const alego_occ_rule* rule, int collapse_z, int unknown_is_obstacle, const alego_occ_inflation* infl, uint8_t* out);
int alego_occ_distance_host(const int8_t* cls, const int32_t n[3], int unknown_is_obstacle, int32_t max_cells, uint32_t* d2, int64_t stats[ALEGO_EDT_STATS]);
int alego_occ_cost_table_host(double s, const alego_occ_inflation* infl, uint8_t* table, int32_t cap);
int alego_occ_costmap_host(const int8_t* cls, const uint32_t* d2, int64_t cells, int unknown_is_obstacle, const uint8_t* table, int32_t n_table, int inflate_unknown,
                           uint8_t* out);

/* ---- static map: the archive's points that the occupancy grid saw through are dropped (csrc/kernels_occ.hip, csrc/occ_math.h; DESIGN.md
 * section 25).  Not part of the reference.  A car that stood somewhere for one key frame stays in the assembled map as a trail of points;
 * the grid holds the evidence against them: their cells were hit once and passed through many times.  Every point of the archive is
 * judged by its OWN cell, against the counts as they stand (the caller integrates first: typically alego_occ_clear, then
 * alego_occ_integrate of all frames with the final poses).  Nothing is allocated or launched without these calls; the archive is not changed.
 *
 * CELL     the point as alego_map_assemble gives it (f32), widened to f64; c_k = floor((x_k - origin_k) / cell_k), the expression that
 *          gives a ray's end cell: after an integration without ranges a point's cell is the cell its own ray hit.
 * VERDICTS one uint8_t per point; the tests are made in this order:
 *   2 OUTSIDE    a coordinate is non-finite, |(x_k - origin_k) / cell_k| > 2^30, or the cell lies outside the grid                kept
 *   3 BELOW      use_keep_below and the point's sensor-frame z (the archived z, f32, z up) < keep_below: ground returns, whose cells
 *                grazing rays pass many times per hit                                                                                kept
 *   0 OCCUPIED   the cell's class under rule.occ is 100                                                                             kept
 *   1 UNKNOWN    the class is -1                                                                                                    kept
 *   4 NEIGHBOUR  the class is 0, protect_radius = r > 0 and a cell of the grid within Chebyshev distance r is of class 100: a wall's
 *                points that fell into the cell next to the wall's own                                                               kept
 *   5 REMOVED    the class is 0 otherwise                                                                                           removed
 * rule = NULL: {{1, 2, 1, 0}, 0, 0, 0, 0}.  ALEGO_ERR_ARG: a negative weight or min_hits, protect_radius outside [0, 2], a non-finite
 * keep_below with use_keep_below set.  Integer and exact f64 arithmetic: device and host agree exactly.
 *
 * alego_occ_mark             returns the number of selected points; verdict[i] belongs to point i of alego_map_assemble(h, slot, kinds & 7,
 *                            leaf 0).  verdict = NULL with cap = 0 only counts (stats is still filled); cap below the count:
 *                            ALEGO_ERR_CAPACITY, nothing written.  stats (may be NULL) gets the number of points per verdict.
 * alego_map_assemble_static  alego_map_assemble's contract (kinds with ALEGO_MAP_FRAME_ID, leaf, count-only, ALEGO_ERR_CAPACITY, return
 *                            value) over the kept points: leaf <= 0 gives the kept points of the raw assembly, in their order and bit for
 *                            bit; leaf > 0 what alego_voxel_grid gives for that cloud.
 * Both are synchronous, behind the slot's own stream, and need a mapping handle with the archive on and the grid enabled.
 * alego_occ_mark_host        the host twin (no device, no handle): pts are world points, sensor_z[i] the sensor-frame z of point i (may be
 *                            NULL when use_keep_below is 0, else ALEGO_ERR_ARG); verdict[n] and stats (may be NULL; set, not added to). */
typedef struct alego_static_rule {
  alego_occ_rule occ;
  int32_t protect_radius;   /* 0..2 */
  int32_t use_keep_below;
  float keep_below;
  int32_t pad;
} alego_static_rule;
enum { ALEGO_STATIC_OCCUPIED = 0, ALEGO_STATIC_UNKNOWN, ALEGO_STATIC_OUTSIDE, ALEGO_STATIC_BELOW, ALEGO_STATIC_NEIGHBOUR, ALEGO_STATIC_REMOVED, ALEGO_STATIC_VERDICTS };
int alego_occ_mark(alego_handle* h, int slot, int kinds, const alego_static_rule* rule, uint8_t* verdict, int32_t cap, int64_t stats[ALEGO_STATIC_VERDICTS]);
int alego_map_assemble_static(alego_handle* h, int slot, int kinds, float leaf, const alego_static_rule* rule, alego_point* out, int32_t cap,
                              int64_t stats[ALEGO_STATIC_VERDICTS]);
int alego_occ_mark_host(const alego_occ_opts* opts, const alego_static_rule* rule, const uint32_t* hits, const uint32_t* passes, const alego_point* pts,
                        const float* sensor_z, int32_t n, uint8_t* verdict, int64_t stats[ALEGO_STATIC_VERDICTS]);

/* ---- one scan-to-map registration sharded over the GPUs of a node (BASELINE.json config 5) ----------------
 * One process per GPU; every rank feeds its handle the SAME scans and so keeps a bit-identical replica of the stream's state
 * (ImageProjection, feature extraction, LaserOdometry and the local map are cheap and are computed redundantly).  What is split
 * is scan2MapOptimization (laserMapping.cpp:360-478): rank r owns the queries [r T / G, (r + 1) T / G) of laser_corner_ds_ ++
 * laser_surf_total_ds_ (5-NN, line / plane fit, residual + Jacobian rows); for every solver evaluation the 28 normal-equation
 * scalars J^T J (21), J^T r (6), cost (1) (+ 2 correspondence counts) are summed with ncclAllReduce(f64) — RCCL over xGMI — on
 * the handle's stream, and every rank takes the identical trust-region step.  The handle must have a single stream group
 * (fewer than 128 slots).  world = 1 is allowed: same kernel sequence, the collective is a copy (hardware tests on one GPU). */
#define ALEGO_DIST_ID_BYTES 128
int alego_dist_unique_id(char id[ALEGO_DIST_ID_BYTES]);   /* rank 0: ncclGetUniqueId; distribute the bytes to every rank */
int alego_dist_init(alego_handle* h, int rank, int world, const char id[ALEGO_DIST_ID_BYTES]);
int alego_dist_shutdown(alego_handle* h);
/* the collective of ONE solver evaluation measured on its own (a mapping frame has ~42 of them): `iters` in-place all-reduces of 32 doubles
 * back to back on the registration's stream; microseconds each.  A collective: every rank of the communicator calls it. */
int alego_dist_allreduce_probe(alego_handle* h, int iters, double* usec_per_allreduce);

/* ---- sensor_msgs/PointCloud2 to alego_point: pcl::fromROSMsg<PointXYZI>, imageProjection.cpp:54-55, IP.cpp:109-110 ----
 * ROS-free mirror of sensor_msgs/PointField + the PointCloud2 layout fields.  Fields are matched by name ("x", "y", "z",
 * "intensity") and must be FLOAT32 (datatype 7) with count 1 (or 0: unset), as PCL's field mapper requires; a missing intensity gives 0.
 * Returns the number of points written (width * height), or ALEGO_ERR_ARG / ALEGO_ERR_CAPACITY. */
typedef struct alego_pc2_field { const char* name; uint32_t offset; uint8_t datatype; uint32_t count; } alego_pc2_field;
int alego_pc2_to_points(const uint8_t* data, uint64_t data_len, uint32_t width, uint32_t height, uint32_t point_step,
                        uint32_t row_step, int is_bigendian, const alego_pc2_field* fields, int n_fields,
                        alego_point* out, int32_t cap);

/* ---- rosbag format 2.0 reader (host side, no ROS / libbz2 / liblz4 needed; csrc/rosbag.cpp) -------------------------------
 * Replaces `rosbag play <file>.bag` + the `/lslidar_point_cloud` subscription + pcl::fromROSMsg at the head of ImageProjection
 * (README.md:33-37, launch/test2.launch:6-14, src/IP.cpp:106-133, src/imageProjection.cpp:45,49-55): open the bag, hand out the
 * messages of a topic in time order, deserialise sensor_msgs/PointCloud2 and run it through alego_pc2_to_points.  Chunks may be
 * uncompressed, bz2 or lz4; a bag without index records (never closed) is scanned.  Errors: ALEGO_ERR_ARG (+ alego_bag_last_error). */
typedef struct alego_bag alego_bag;
int alego_bag_open(const char* path, alego_bag** out);
void alego_bag_close(alego_bag* b);
const char* alego_bag_last_error(const alego_bag* b);
int alego_bag_topic_count(const alego_bag* b);
int alego_bag_topic_info(const alego_bag* b, int i, const char** topic, const char** datatype, int64_t* n_messages);
int64_t alego_bag_message_count(const alego_bag* b, const char* topic);
/* serialized message `index` of `topic` (pointer valid until the next read / close); bag_time = the record's receive time */
int alego_bag_read_raw(alego_bag* b, const char* topic, int64_t index, const uint8_t** data, uint64_t* len, double* bag_time);
/* PointCloud2 message `index` of `topic` -> points (returns their number); header_stamp = msg.header.stamp, is_dense = msg.is_dense */
int alego_bag_read_pc2(alego_bag* b, const char* topic, int64_t index, alego_point* out, int32_t cap, double* header_stamp, int32_t* is_dense);

#ifdef __cplusplus
}
#endif
#endif /* ALEGO_MI355X_H_ */
