// lm_host.h — LaserMapping scan-to-map registration: host sequencing + HBM state.
#ifndef ALEGO_LM_HOST_H_
#define ALEGO_LM_HOST_H_
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_common.h"

struct LmHost;
LmHost* lm_host_create(const alego_params& P, const DevCtx& d, int n_slots, int gsize, const std::vector<hipStream_t>& streams, std::string* err);
void lm_host_destroy(LmHost* lm);
// LaserMapping for the scan just processed by LO, for the slots of view `d`
// st_override: enqueue on this stream instead of the slot's group stream (alego_stream_run pipelines LaserMapping on a stream of its own)
int lm_host_enqueue(LmHost* lm, const DevCtx& d, const std::vector<char>& odom_valid, std::string* err, hipStream_t st_override = nullptr);
// the batch path: LaserMapping of this scan on `back`, behind the hand-over kernel (lm_stage) on `front`; k = scans handed over so far for
// this stream group, back_same / back_other = events recorded on `back` after the LaserMapping of scans k - 2 / k - 1
int lm_host_enqueue_async(LmHost* lm, const DevCtx& d, const std::vector<char>& odom_valid, std::string* err, hipStream_t front, hipStream_t back,
                          hipEvent_t staged, hipEvent_t back_same, hipEvent_t back_other, long k);
const double* lm_host_stage_odom(LmHost* lm);   // the odometry lm_stage handed over (device, [slot][2][8])
int lm_host_get_flags(LmHost* lm, int slot);
int lm_host_process_host(LmHost* lm, const DevCtx& d, const alego_point* corner_last, int n_corner, const alego_point* surf_last,
                         int n_surf, const alego_point* outlier, int n_outlier, const alego_pose* odom, alego_pose* map_pose,
                         std::string* err);
void lm_host_get_params(LmHost* lm, int slot, double* p6);
int lm_host_set_params(LmHost* lm, int slot, const double* p6, std::string* err);
void lm_host_get_counts(LmHost* lm, int slot, int* out6);
int lm_host_keyframe_count(LmHost* lm, int slot);
int lm_host_get_keyframe(LmHost* lm, int slot, int kf_id, alego_keyframe* out, std::string* err);
int lm_host_set_keypose(LmHost* lm, const DevCtx& d, int slot, int kf_id, const float* pose6, std::string* err);
int lm_host_reset_window(LmHost* lm, int slot, std::string* err);
int lm_host_apply_correction(LmHost* lm, const DevCtx& d, int slot, const double* rc12, std::string* err);
int lm_host_add_keyframe(LmHost* lm, const DevCtx& d, int slot, const float* pose6, const alego_point* corner, int nc, const alego_point* surf, int ns,
                         const alego_point* outlier, int no, std::string* err);
int lm_host_dist_unique_id(char* id128);
int lm_host_dist_init(LmHost* lm, int rank, int world, const char* id128, std::string* err);
int lm_host_dist_shutdown(LmHost* lm);
int lm_host_dist_probe(LmHost* lm, int iters, double* usec, std::string* err);
int lm_host_debug_slice(LmHost* lm, int rank, int world, std::string* err);
int lm_host_set_map_merge(LmHost* lm, int on, std::string* err);
int lm_host_debug_get(LmHost* lm, int slot, const char* name, void* out, int cap_bytes, int* count, int* dtype, std::string* err);
// the global map (include/alego_mi355x.h: alego_map_*, alego_lm_get_local_map, alego_voxel_grid)
int lm_host_map_enable(LmHost* lm, int max_frames, int max_points, std::string* err);
int lm_host_map_status(LmHost* lm, int slot, int* out4, std::string* err);
int lm_host_map_set_keyposes(LmHost* lm, int slot, int first, int n, const float* poses6, std::string* err);
int lm_host_map_get_keyframe(LmHost* lm, int slot, int id, alego_keyframe* out, std::string* err);
// stamps of archived frames first .. first + n - 1: read (write = 0) or overwrite (write = 1)
int lm_host_map_stamps(LmHost* lm, int slot, int first, int n, double* stamps, int write, std::string* err);
// the stamped entry points (alego_scan_process / alego_lo_process): the slot's archived frames take DevCtx::scan_stamp from now on
int lm_host_map_mark_stamped(LmHost* lm, int slot, hipStream_t st);
struct LmCtx;
const LmCtx* lm_host_ctx(LmHost* lm);   // the device view (the batched loop-closure search reads the archive through it)
int lm_host_map_assemble(LmHost* lm, int slot, int kinds, float leaf, alego_point* out, int cap, std::string* err);
int lm_host_map_keyposes(LmHost* lm, int slot, alego_point* out, int cap, std::string* err);
// the occupancy grid (alego_occ_*; kernels_occ.hip); the caller has checked that the grid exists (lm_host_occ_on) before every call but enable
bool lm_host_occ_on(LmHost* lm);
int lm_host_occ_enable(LmHost* lm, const alego_occ_opts* opts, std::string* err);
int lm_host_occ_clear(LmHost* lm, std::string* err);
int lm_host_occ_integrate(LmHost* lm, int slot, int first, int n, int kinds, int64_t* stats, std::string* err);
int lm_host_occ_get(LmHost* lm, uint32_t* hits, uint32_t* passes, std::string* err);
int lm_host_occ_classify(LmHost* lm, const alego_occ_rule& rule, int collapse_z, int8_t* out, std::string* err);
int lm_host_occ_set_piece(LmHost* lm, int piece);   // alego_debug_occ_piece
// the clearance field and the cost map (alego_occ_distance / alego_occ_costmap; kernels_edt.hip); d2 / stats may be null
int lm_host_occ_set(LmHost* lm, const uint32_t* hits, const uint32_t* passes, std::string* err);
int lm_host_occ_distance(LmHost* lm, const alego_occ_rule& rule, const alego_occ_dist_opts& o, uint32_t* d2, int64_t* stats, std::string* err);
int lm_host_occ_costmap(LmHost* lm, const alego_occ_rule& rule, int collapse_z, int unknown_is_obstacle, const alego_occ_inflation& infl, uint8_t* out, std::string* err);
// the static map: verdicts of every selected point of `slot` (returns their number), and the assembly without the removed points
int lm_host_occ_mark(LmHost* lm, int slot, int kinds, const alego_static_rule& rule, uint8_t* verdict, int cap, int64_t* stats, std::string* err);
int lm_host_map_assemble_static(LmHost* lm, int slot, int kinds, float leaf, const alego_static_rule& rule, alego_point* out, int cap, int64_t* stats, std::string* err);
int lm_host_get_local_map(LmHost* lm, int slot, alego_point* corner, int corner_cap, alego_point* surf, int surf_cap, int* n_out, std::string* err);
int lm_host_voxel_grid(LmHost* lm, hipStream_t st, const alego_point* pts, int n, float leaf, alego_point* out, int cap, std::string* err);
int lm_host_set_gv_small_max(LmHost* lm, int v);
// the key-pose graph (alego_graph_*; kernels_graph.hip)
int lm_host_graph_enable(LmHost* lm, int max_loops, const double* odom_var6, std::string* err);
// correctPoses for the slots with apply[slot] != 0 (apply_dev: the same flags on the device); n_poses_max: most key frames of an applied slot
int lm_host_graph_apply(LmHost* lm, const std::vector<int>& apply, const int* apply_dev, int n_poses_max, std::string* err);
// a slot moved / one archive appended to another's on the device (alego_map_move / alego_map_merge; kernels_merge.hip); arguments checked by the caller
struct PgCtx;
int lm_host_map_move(LmHost* lm, const int* slots, int n, const double* T12, int* out_status, std::string* err);
int lm_host_map_merge(LmHost* lm, PgCtx** pc, const int* src, const int* dst, int n, const double* T12, double stamp_off, const double* seam_var6,
                      const alego_map_align_hyp* hyp, alego_map_merge_result* out, std::string* err);
// a slot's archive thinned in place (alego_map_thin; kernels_thin.hip); arguments checked by the caller.  first_dropped[i]: the first dropped id of
// slots[i] (its frame count when none was dropped).  debug_thin_select: th_select alone on the caller's arrays, returns the frames kept
int lm_host_map_thin(LmHost* lm, const int* slots, int n, double min_dist, alego_map_thin_result* out, int* first_dropped, std::string* err);
int lm_host_debug_thin_select(LmHost* lm, const float* keyposes6, const uint8_t* protect, int n, double min_dist, uint8_t* keep, std::string* err);
// localisation mode (alego_loc_*; kernels_loc.hip): the frozen map store shared by every slot
int lm_host_loc_enable(LmHost* lm, const DevCtx& d, const alego_kf_in* frames, int n, double radius, std::string* err);
// ... built on the device from the archive of `slot` of the mapping handle `src` as it is now, in chunks (the caller has synchronised every stream of both
// handles); capacity: frames the store is allocated for (<= 0: the archived frames).  update: the store of a handle that localises is rebuilt from it
int lm_host_loc_enable_from_map(LmHost* lm, const DevCtx& d, LmHost* src, int slot, double radius, int capacity, std::string* err);
int lm_host_loc_update_from_map(LmHost* lm, LmHost* src, int slot, bool* rewritten, std::string* err);   // rewritten: the store was touched (it is empty after a failure then)
int lm_host_set_loc_chunk(LmHost* lm, int frames);   // ALEGO_LOC_CHUNK: frames per chunk of that build
int lm_host_loc_status(LmHost* lm, int slot, int* out4, std::string* err);
bool lm_host_localising(LmHost* lm);
// covariance of the registration (alego_regcov_*; lm_regcov in kernels_lm.hip).  The caller has synchronised the handle's streams before enable.
int lm_host_regcov_enable(LmHost* lm, const alego_regcov_opts* opts, std::string* err);
int lm_host_regcov_get(LmHost* lm, const int* slots, int n, alego_regcov* out, std::string* err);
bool lm_host_regcov_on(LmHost* lm);
// solution remapping (alego_remap_*; lm_solve_remap in kernels_lm.hip), as above
int lm_host_remap_enable(LmHost* lm, const alego_remap_opts* opts, std::string* err);
int lm_host_remap_get(LmHost* lm, const int* slots, int n, alego_remap* out, std::string* err);
double lm_host_remap_eig_min(LmHost* lm);   // the handle's resolved option (the default while the feature is off; lm may be null)
bool lm_host_regcov_opts(LmHost* lm, double* opt16);   // the handle's resolved options (the defaults while the feature is off; lm may be null); true: the feature is on
#endif
