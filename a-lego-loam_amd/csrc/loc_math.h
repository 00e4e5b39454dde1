// loc_math.h — the window selection rule of localisation mode, shared by the kernel (loc_select, kernels_loc.hip) and the host
// restatement (alego_loc_select): one definition, so the two cannot drift apart.
//
// p is the f32 of t_map2laser_ after transformAssociateToMap.  Frame i of the frozen map is a CANDIDATE when the f32 squared distance of
// its key pose to p, accumulated as lc_detect accumulates it (kernels_loop.hip; no contraction: the build has -ffp-contract=off), is below
// (float)(radius * radius).  Of the candidates the K smallest in the order (d², id) are kept: nn_rules.h's distance, radius test and key, which
// is unique per frame.  The window is their ids in ascending order.  A non-finite p selects
// nothing.  This rule is the project's own, not the reference's surround-key-frame bookkeeping.
#ifndef ALEGO_LOC_MATH_H_
#define ALEGO_LOC_MATH_H_
#include "nn_rules.h"

#ifdef __HIPCC__
#define LOC_FN __host__ __device__ inline
#else
#define LOC_FN inline
#endif

#define LOC_DEFAULT_RADIUS 50.0   // surround_keyframe_search_radius_ (LM.cpp:183)
// Frames of a map store.  loc_select's worst case (more than K candidates) recomputes every key in each of K rounds: 8192 frames at the
// largest K (512) are 16 k key evaluations per thread and frame, the size this was written for; map_accum's 16-bit window entries allow 65535.
#define LOC_MAX_FRAMES 8192

LOC_FN float loc_r2(double radius) {
  const double r = radius > 0.0 ? radius : LOC_DEFAULT_RADIUS;
  return nn_r2(r);
}
LOC_FN float loc_d2(const float* kp, float px, float py, float pz) { return nn_d2(kp[0], kp[1], kp[2], px, py, pz); }
LOC_FN bool loc_finite(float v) { return v - v == 0.f; }
// the key of frame `id`, or NN_NONE when it is no candidate
LOC_FN unsigned long long loc_key(const float* kp, int id, float px, float py, float pz, float r2) {
  const float d2 = loc_d2(kp, px, py, pz);
  return nn_in_radius(d2, r2) ? nn_key(d2, (uint32_t)id) : NN_NONE;
}

#endif
