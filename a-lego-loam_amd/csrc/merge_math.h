// merge_math.h — the arithmetic of alego_map_move / alego_map_merge, shared by the kernels (kernels_merge.hip) and the
// host twins (alego_map_align_poses, alego_map_merge_edges): one definition, so the two cannot drift apart.  Plain C++ that a host compiler
// reads without the HIP runtime; f64 without contraction (-ffp-contract=off).
//
// MOVED POSE: the f32 key pose of T * Pose3(RzRyRx(roll, pitch, yaw), xyz): pg_from_pose6, the f64 product (pg_compose), pg_to_pose6.  The
// products and sums are the same f64 on both sides; sin, cos and atan2 come from two libraries (the device's and the host's), so a component
// may differ in its last f32 bit between the two.
// MOVED PRIOR: between <- T * between (pg_compose), what keeps a moved slot's graph where the move put it.
// MERGED CHAIN: behind a destination of nd frames, edge nd (the seam) is the prior on the first moved pose (nd == 0) or
// between(destination pose nd - 1, first moved pose), both as Pose3 of their f32 key poses - the rule of map_archive - with the seam's
// variances; edge nd + f (f >= 1) is the source's chain edge f with both ids raised by nd: a measurement stays what was measured.
// MERGED LOOPS: the source's loop edges in their order, ids raised by nd.
#ifndef ALEGO_MERGE_MATH_H_
#define ALEGO_MERGE_MATH_H_
#include <stdint.h>

#include "../../include/alego_mi355x.h"
#include "pg_math.h"

// points of one work item of the archive-to-archive copy (ALEGO_MERGE_COPY_ITEM): 256 lanes x 4 x 16 B
#define MG_ITEM ALEGO_MERGE_COPY_ITEM
#define MG_T 256

PG_FN void mg_move_pose6(const double* T12, const float* in6, float* out6) {
  double X[12], Y[12];
  pg_from_pose6(in6, X);
  pg_compose(T12, X, Y);
  pg_to_pose6(Y, out6);
}
PG_FN void mg_move_prior(const double* T12, const double* between, double* out12) {
  double Y[12];
  pg_compose(T12, between, Y);
  for (int k = 0; k < 12; ++k) out12[k] = Y[k];
}
// the seam: chain edge nd of the merged destination; prev6 = the destination's key pose nd - 1 (unused when nd == 0), first6 = the first moved pose
PG_FN void mg_seam_edge(int nd, const float* prev6, const float* first6, const double* var6, alego_graph_edge* e) {
  double xn[12];
  pg_from_pose6(first6, xn);
  e->from = nd - 1; e->to = nd;
  if (nd == 0) {
    for (int k = 0; k < 12; ++k) e->between[k] = xn[k];
  } else {
    double xp[12];
    pg_from_pose6(prev6, xp);
    pg_between(xp, xn, e->between);
  }
  for (int k = 0; k < 6; ++k) e->variance[k] = var6[k];
}
// an edge of the source with both ids raised by nd
PG_FN void mg_shift_edge(const alego_graph_edge* in, int nd, alego_graph_edge* out) {
  *out = *in;
  out->from = in->from + nd; out->to = in->to + nd;
}
PG_FN bool mg_finite12(const double* T12) {
  for (int k = 0; k < 12; ++k) if (!(T12[k] - T12[k] == 0.0)) return false;
  return true;
}
#endif
