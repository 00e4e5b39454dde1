// front_end.h — host entry points of the front end (ImageProjection, feature extraction, LaserOdometry): the launchers, the probes of
// the alego_debug_* calls and the one-time kernel configuration, each defined in the file named.
#ifndef ALEGO_FRONT_END_H_
#define ALEGO_FRONT_END_H_
#include "dev_common.h"

// kernels_ip.hip, kernels_ipf.hip, kernels_ipb.hip
void launch_ip(const DevCtx& d, int ring_pos, bool want_labels, hipStream_t st);
void launch_atan2f_probe(const float* y, const float* x, float* out, int n, int mode, hipStream_t st);
int ip_configure(const DevCtx& d);
bool ipf_eligible(const DevCtx& d), ipw_eligible(const DevCtx& d), ipb_eligible(const DevCtx& d);
void launch_ip_fused(const DevCtx& d, int ring_pos, bool keep_images, hipStream_t st);
int ipf_configure(const DevCtx& d);
void launch_ipb(const DevCtx& d, int ring_pos, bool keep_images, hipStream_t st);
// kernels_fe.hip, kernels_fe2.hip
void launch_fe(const DevCtx& d, hipStream_t st);
void launch_fe_curv_debug(const DevCtx& d, hipStream_t st);   // fe_curv alone (curvature sums / occlusion marks of the points outside every sector, tests only)
int launch_stdsort_probe(const uint32_t* keys, int n, int depth_limit, int* pos_out, hipStream_t st);
bool fe_fused_eligible(const DevCtx& d);
int fe_cand_span(const DevCtx& d);    // sectors of a ring per fe_cand wavefront as the handle runs it (0: the whole ring; alego_debug_get "fe_cand_span")
int fe_sector_cap(const DevCtx& d);   // entries of a ring sector's candidate list (fe_cand; alego_debug_get "fe_cand_lists")
void launch_fe_fused(const DevCtx& d, hipStream_t st);
// kernels_lo.hip
void launch_lo(const DevCtx& d, hipStream_t st);
void launch_lo_grid(const DevCtx& d, hipStream_t st);   // the target grid of the clouds just written, for the next scan's LaserOdometry
void launch_lo_imu_push(const DevCtx& d, int slot, const double* smp_dev, int n, hipStream_t st);
void launch_lo_deskew(const DevCtx& d, hipStream_t st);
void launch_traj_log(const DevCtx& d, hipStream_t st, const double* staged_odom = nullptr, int par = 0);
void launch_dbg_eval_blocks(int type, int n, const double* geom13, const double* params6, double* res, double* jac6, hipStream_t st);
void launch_dbg_transform_to_start(const double* params6, const float4* pts, int n, float4* out, hipStream_t st);
int lo_configure();
#endif
