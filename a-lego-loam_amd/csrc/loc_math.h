// loc_math.h — the window selection rule of localisation mode, shared by the kernel (loc_select, kernels_loc.hip) and the host
// restatement (alego_loc_select): one definition, so the two cannot drift apart.
//
// p is the f32 of t_map2laser_ after transformAssociateToMap.  Frame i of the frozen map is a CANDIDATE when the f32 squared distance of
// its key pose to p, accumulated as lc_detect accumulates it (kernels_loop.hip; no contraction: the build has -ffp-contract=off), is below
// (float)(radius * radius).  Of the candidates the K smallest in the order (d² bits, id) are kept — d² >= 0, so its bit pattern orders it
// and the packed 64-bit key (bits << 32 | id) is unique per frame.  The window is their ids in ascending order.  A non-finite p selects
// nothing.  This rule is the project's own, not the reference's surround-key-frame bookkeeping.
#ifndef ALEGO_LOC_MATH_H_
#define ALEGO_LOC_MATH_H_
#include <stdint.h>
#include <string.h>

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
  return (float)(r * r);
}
LOC_FN float loc_d2(const float* kp, float px, float py, float pz) {
  float r = 0.f, df;
  df = kp[0] - px; r += df * df; df = kp[1] - py; r += df * df; df = kp[2] - pz; r += df * df;
  return r;
}
LOC_FN bool loc_finite(float v) { return v - v == 0.f; }
// the packed key of frame `id`, or ~0 when it is no candidate
LOC_FN unsigned long long loc_key(const float* kp, int id, float px, float py, float pz, float r2) {
  const float d2 = loc_d2(kp, px, py, pz);
  if (!(d2 < r2)) return ~0ull;
  uint32_t bits;
  memcpy(&bits, &d2, sizeof(bits));
  return ((unsigned long long)bits << 32) | (uint32_t)id;
}

#endif
