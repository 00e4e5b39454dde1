// thin_math.h — the rule of alego_map_thin, shared by the kernels (kernels_thin.hip) and the host twins
// (alego_map_thin_select, alego_map_thin_edges): one definition, so the two cannot drift apart.  Plain C++ that a host compiler reads
// without the HIP runtime; no contraction (-ffp-contract=off).  The rule is the project's own.
//
// SELECTION: frames are visited in id order.  A PROTECTED frame is always kept.  An unprotected frame i is dropped iff some KEPT frame
// j < i lies closer than min_dist: the f32 squared distance of the two key-pose positions, accumulated as loc_d2 accumulates it
// (((dx dx) + dy dy) + dz dz, loc_math.h), is < (float)(min_dist * min_dist).  A non-finite position makes every comparison false: such
// a frame is kept and suppresses nothing.  min_dist <= 0 drops nothing.  Position only, no trigonometry: device and host agree bit for
// bit.  The rule is greedy - a dropped frame suppresses nobody - and "some kept j < i" does not depend on the order the kept frames
// are tested in, so testing one frame against all earlier kept frames in parallel is exact.
// CHAIN: with the kept ids k_0 = 0 < k_1 < ..., new chain edge m (m - 1 -> m) has the f64 product of the old chain measurements
// k_(m-1) + 1 .. k_m, in that order, associated left to right (pg_compose), and as variances the component-wise sums of the composed
// edges' variances, summed in the same order.  That sum is a FIRST-ORDER rule: it ignores how the intermediate rotations mix the
// components (the exact propagation would carry every covariance through the adjoint of the edges behind it).  A run of one edge is
// that edge, bit for bit: a measurement stays what was measured.  Edge 0, the prior, is unchanged.
// LOOPS: a loop edge keeps its measurement and variances; both ids go through the old -> new id table.
#ifndef ALEGO_THIN_MATH_H_
#define ALEGO_THIN_MATH_H_
#include <stdint.h>

#include "../../include/alego_mi355x.h"
#include "loc_math.h"
#include "pg_math.h"

// kept positions th_select holds in LDS (3 x 4 B each); the kept frames beyond them are read from the poses
#define TH_LDS_KEPT 2048

// the threshold d2 is compared with; -1 (no d2 is below it) when min_dist drops nothing
PG_FN float th_r2(double min_dist) { return min_dist > 0.0 ? (float)(min_dist * min_dist) : -1.f; }
// kept frame at (jx, jy, jz) suppresses the unprotected frame with key pose ki
PG_FN bool th_suppresses(float jx, float jy, float jz, const float* ki, float r2) { return loc_d2(ki, jx, jy, jz) < r2; }

// the host's greedy pass: poses[i * stride + 0 .. 2] = position of frame i; keep[n] is written; returns the frames kept
inline int th_select_host(const float* poses, int stride, const uint8_t* protect, int n, double min_dist, uint8_t* keep) {
  const float r2 = th_r2(min_dist);
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    bool drop = false;
    if (!(protect && protect[i])) {
      const float* ki = poses + (size_t)i * stride;
      for (int j = 0; j < i && !drop; ++j)
        if (keep[j]) { const float* kj = poses + (size_t)j * stride; drop = th_suppresses(kj[0], kj[1], kj[2], ki, r2); }
    }
    keep[i] = drop ? 0 : 1;
    kept += keep[i];
  }
  return kept;
}

// new chain edge m from the old chain edges a + 1 .. b (a = the kept frame before b; a < b)
PG_FN void th_compose_edge(const alego_graph_edge* chain, int a, int b, int m, alego_graph_edge* out) {
  alego_graph_edge e = chain[a + 1];
  for (int f = a + 2; f <= b; ++f) {
    double Y[12];
    pg_compose(e.between, chain[f].between, Y);
    for (int k = 0; k < 12; ++k) e.between[k] = Y[k];
    for (int k = 0; k < 6; ++k) e.variance[k] += chain[f].variance[k];
  }
  e.from = m - 1; e.to = m;
  *out = e;
}
// a loop edge under the old -> new id table (new_id[f] < 0: f was dropped); false when an endpoint has no new id
PG_FN bool th_remap_edge(const alego_graph_edge* in, const int* new_id, int n, alego_graph_edge* out) {
  const int a = in->from, b = in->to;
  if (a < 0 || a >= n || b < 0 || b >= n || new_id[a] < 0 || new_id[b] < 0) return false;
  alego_graph_edge e = *in;
  e.from = new_id[a]; e.to = new_id[b];
  *out = e;
  return true;
}
#endif
