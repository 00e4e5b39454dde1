// nn_rules.h — the arithmetic of every nearest-neighbour search: the squared distance, the order key, the lower bounds of "distance to a box",
// the cells of the three grids, the gates, and the rules of LaserOdometry's ring walk.  lo_grid_build / lo_assoc (kernels_lo.hip), lm_grid_build /
// lm_knn (kernels_lm.hip), lc_detect / lc_grid_build / lc_nn (kernels_loop.hip), icp_nn (kernels_icp.hip), loc_math.h and alego_loop_detect take their
// rules from here; each rule, the reference lines it restates and the argument why the search stays EXACT are stated here once.  Plain numbers in.
// Readable by a host compiler without the HIP runtime: tests/nn_rules/nn_rules_check.cpp checks every rule against its plain statement, on the CPU.
// Built with -ffp-contract=off everywhere.  Two facts carry every argument below: an IEEE operation rounds monotonically (a <= b in real numbers
// gives fl(a) <= fl(b)), and fl(a - b) = -fl(b - a).
#ifndef ALEGO_NN_RULES_H_
#define ALEGO_NN_RULES_H_
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define NN_RULE_FN __host__ __device__ __forceinline__
#else
#define NN_RULE_FN inline
#endif
NN_RULE_FN uint32_t nn_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
NN_RULE_FN float nn_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---- distance: flann::L2_Simple<float> (what pcl::KdTreeFLANN compares and returns) --------------------------------------------------------------
// r = 0; r += dx * dx; r += dy * dy; r += dz * dz in f32, x first.  The sign of a difference does not matter (fl(a - b) = -fl(b - a), and the
// square drops it), so a call site may subtract either way.  0 + dx² = dx² exactly, so the grouping (dx² + dy²) + dz² has the same bits: that
// is nn_d2_pk, lm_knn's form on packed pairs.  The result is never -0 and is NaN only for a non-finite input or an infinite difference.
NN_RULE_FN float nn_d2(float ax, float ay, float az, float bx, float by, float bz) {
  float r = 0.f, df;
  df = ax - bx; r += df * df; df = ay - by; r += df * df; df = az - bz; r += df * df;
  return r;
}
#if defined(__HIPCC__)
// v_pk_add_f32 / v_pk_mul_f32 are IEEE operations on both halves: 6 instead of 8 VALU instructions per candidate
typedef float nn_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float nn_d2_pk(nn_v2f axy, float az, nn_v2f bxy, float bz) {
  const nn_v2f dxy = axy - bxy, sq = dxy * dxy;
  const float dz = az - bz;
  float r = sq.x + sq.y;
  r += dz * dz;
  return r;
}
#endif

// ---- key: the (d², index) order, ties to the lowest index, as one unsigned integer ------------------------------------------------------------------
// The bit pattern of a float >= +0 orders like its value (+inf included), so for d² >= 0 and 0 <= index < 2^31 the integer order of
// nn_key is the lexicographic order of (d², index), and a minimum over keys — lane-private, then cross-lane — is the arg-min whatever the visiting
// order.  NN_NONE ("no neighbour yet") is above every key of a d² that is not NaN.
typedef unsigned long long nn_key_t;
#define NN_NONE (~0ull)
NN_RULE_FN nn_key_t nn_key(float d2, uint32_t index) { return ((nn_key_t)nn_f32_bits(d2) << 32) | index; }
NN_RULE_FN float nn_key_d2(nn_key_t k) { return nn_bits_f32((uint32_t)(k >> 32)); }
NN_RULE_FN int nn_key_index(nn_key_t k) { return (int)(uint32_t)k; }
// The pair form of the same order: candidate (d, i) beats the best (bd, bi).  For d, bd >= 0 (no NaN) and indices >= 0 it is nn_key(d, i) <
// nn_key(bd, bi).  The two differ only at the start state.  A key search starts at NN_NONE and takes any first candidate, +inf and NaN included;
// lc_nn and icp_nn start at (FLT_MAX, -1), where a candidate at exactly FLT_MAX (no index is below -1), +inf or NaN (no comparison holds)
// stays "no neighbour", as their callers expect (an index of -1 with d² = FLT_MAX).  A call site that changes form must keep its start state's rule.
// Candidates visited in ascending index need only d < bd: the tie term is never true (icp_nn).
NN_RULE_FN bool nn_better(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// ---- bounds: a lower bound of the distance to every point of an axis-aligned box [lo, hi] --------------------------------------------------------
// The gap of one axis, 0 inside: for a point p of the box, lo <= p <= hi, either q <= p and lo - q <= p - q, or q > p and q - hi <= q - p; the
// other term is <= 0.  Rounding is monotone, so nn_gap <= |fl(p - q)| in the precision the gap is taken in.
NN_RULE_FN float nn_gap(float lo, float hi, float q) { return fmaxf(fmaxf(lo - q, q - hi), 0.f); }
NN_RULE_FN double nn_gap_f64(float lo, float hi, float q) { return fmax(0.0, fmax((double)lo - (double)q, (double)q - (double)hi)); }
// LaserOdometry's 1-NN bound: nn_d2's own operations on the gaps (squares of non-negative numbers and sums are monotone too), so the bound is
// <= nn_d2 of every point of the box, in f32, bit for bit: a box whose bound exceeds the best d² holds no point that could win or tie.
NN_RULE_FN float nn_box_lb(float gx, float gy, float gz) { float r = 0.f; r += gx * gx; r += gy * gy; r += gz * gz; return r; }
// The loop ICP's bound: gaps and sum in f64 — a lower bound of the REAL distance to the box, not of its f32 value.  nn_d2 is below the real
// d² by less than 4e-7 of it (the roundings of the differences, the squares and the two sums together) or, when a square underflows, by
// less than 1e-37: a cell is skipped only when the bound shrunk by NN_PRUNE and that much still EXCEEDS the best d², so every point of it has
// an f32 d² strictly larger and cannot win or tie.
#define NN_PRUNE 0.999999
NN_RULE_FN double nn_box_lb_f64(double gx, double gy, double gz) { return gx * gx + gy * gy + gz * gz; }
NN_RULE_FN bool nn_beyond(double lb, float best_d2) { return lb * NN_PRUNE - 1e-37 > (double)best_d2; }
// ... and its bound to the half-space beyond a face of the visited block of cells: the distance to the face less the face's slack, squared.  The
// faces are mn + c * h in f64 (nn_lc_axis below); the slack covers what that sum and x - mn can round by.
NN_RULE_FN double nn_face_slack(double mn, double extent, double h) { return 1e-12 * (fabs(mn) + extent + h); }
NN_RULE_FN double nn_face_lb(double to_face, double slack) { const double d = fmax(0.0, to_face - slack); return d * d; }

// ---- cells ---------------------------------------------------------------------------------------------------------------------------------
// LaserOdometry's 2-D grid over (x, y): origin = the cloud's minimum, cells of csz = 2^k metres (inv = 1 / csz, exact), at most LO_GC cells, so
// fewer than 2^12 along an axis.  lo_grid_build clamps the coordinate into the grid (the origin and the extent come from the boxes of the
// cloud, which hold every target: the clamp moves none); lo_assoc does not clamp the query's and looks at the cells within one of it.
// x - origin rounds by at most 2^-13 cell there, target and query together 2^-12: a target with f32 d² < 0.999 csz² has |dx| < 0.9995 csz in real
// numbers (the roundings of nn_d2 move that by 1e-7), its coordinate differs from the query's by less than 1 and its cell by at most one — such
// a target lies in the 3 x 3 cells, so a best candidate below the settle threshold IS the nearest neighbour.
NN_RULE_FN int nn_lo_cell(float x, float origin, float inv) { return (int)floorf((x - origin) * inv); }
NN_RULE_FN float nn_lo_settle(float csz) { return 0.999f * csz * csz; }
// LaserMapping's 3-D lattice: the cell of x is floorf(x * inv) with inv = 1 / cell a power of two, so x * inv and its floor are exact and every
// point lies in its true cell of a global lattice (floorf((x - ox) * inv) with a float origin rounds in the subtraction: across a binade boundary
// a point at f32 d² < cell² could sit two cells from the query).  The float is clamped before the conversion: any finite input gives a defined int.
// cell² >= knn_max_dist (nn_lm_cell), and lm_knn keeps only candidates with d² < knn_max_dist (nn_lm_limit_bits): then |dx| < cell along every
// axis in real numbers (rounding is monotone, cell² is a power of two) and the candidate is at most one cell from the query: 27 cells suffice.
NN_RULE_FN int nn_lm_coord(float x, float inv) { return (int)fminf(fmaxf(floorf(x * inv), -1073741824.0f), 1073741824.0f); }
NN_RULE_FN float nn_lm_cell(double knn_max_dist) { float cell = 1.0f; while ((double)cell * cell < knn_max_dist) cell *= 2.0f; return cell; }
NN_RULE_FN int nn_clampi(int v, int lo, int hi) { const int t = v < lo ? lo : v; return t > hi ? hi : t; }   // min(max(v, lo), hi)
// the clamped linear cell of lattice coordinates relative to the grid's origin cell (map points are never clamped: lm_grid_build's margin)
NN_RULE_FN int nn_lm_index(int ix, int iy, int iz, int gx, int gy, int gz) {
  return nn_clampi(ix, 0, gx - 1) + gx * (nn_clampi(iy, 0, gy - 1) + gy * nn_clampi(iz, 0, gz - 1));
}
// The loop grid: cells of h = 2^k from the target's minimum, the coordinate floor((x - mn) * 2^-k) in f64 clamped into the grid (NaN -> 0).
// x - mn of two f32 is exact in f64 unless their exponents differ by more than 29, and the scaling is exact: nn_face_slack covers the rest.
NN_RULE_FN int nn_lc_axis(float x, double mn, double inv_h, int g) {
  double v = floor(((double)x - mn) * inv_h);
  if (!(v >= 0.0)) v = 0.0;
  if (v > (double)(g - 1)) v = (double)(g - 1);
  return (int)v;
}
NN_RULE_FN int nn_lc_index(int ix, int iy, int iz, int gx, int gy) { return (iz * gy + iy) * gx + ix; }
// the smallest k for which the extents e[] (largest: emax) make at most `target` cells of 2^k; 2^k > every extent is one cell
NN_RULE_FN int nn_lc_cell_exp(const double e[3], double emax, double target) {
  int k = emax > 0.0 ? ilogb(emax) + 1 : 0;
  for (int it = 0; it < 160; ++it) {   // halve while the cell count stays within the target
    const double h2 = ldexp(1.0, k - 1);
    double cnt = 1.0;
    for (int a = 0; a < 3; ++a) cnt *= floor(e[a] / h2) + 1.0;
    if (cnt > target || k - 1 < -120) break;
    --k;
  }
  return k;
}

// ---- gates ---------------------------------------------------------------------------------------------------------------------------------
// LaserMapping accepts a query when its FIFTH neighbour is closer than knn_max_dist, compared in double (laserMapping.cpp:376,:426): a
// neighbour at knn_max_dist or beyond is part of no accepted row and need not enter a top-5 set.  The limit is the bit pattern of the smallest
// f32 f with (double)f >= knn_max_dist, so that for d² >= 0: bits(d²) < limit  <=>  (double)d² < knn_max_dist (0: nothing passes).
NN_RULE_FN uint32_t nn_lm_limit_bits(double knn_max_dist) {
  float flim = (float)knn_max_dist;
  if ((double)flim < knn_max_dist) flim = nn_bits_f32(nn_f32_bits(flim) + 1);
  return knn_max_dist > 0.0 ? nn_f32_bits(flim) : 0u;
}
NN_RULE_FN bool nn_lm_within(float d2, uint32_t limit_bits) { return nn_f32_bits(d2) < limit_bits; }
// i5, d5: index (-1: none, NN_NONE's) and d² of the fifth neighbour
NN_RULE_FN bool nn_lm_row_ok(int i5, float d5, double knn_max_dist) { return i5 != -1 && (double)d5 < knn_max_dist; }
// LaserOdometry: search_dist[0] < nearest_feature_dist, float against double (laserOdometry.cpp:343,:433)
NN_RULE_FN bool nn_lo_found(float d2, double nearest_feature_dist) { return (double)d2 < nearest_feature_dist; }
// radiusSearch (laserMapping.cpp:778; loc_select's and the thinning's rule): f32 d² below the f32 of the squared radius
NN_RULE_FN float nn_r2(double radius) { return (float)(radius * radius); }
NN_RULE_FN bool nn_in_radius(float d2, float r2) { return d2 < r2; }

// ---- LaserOdometry's ring walk (laserOdometry.cpp:344-373 surf, :433-475 corner) -------------------------------------------------------------------
// From the closest point the reference walks up (closest + 1, + 2, ...) until a ring above closest's + ring_window, then down (closest - 1,
// - 2, ...) until one below it, and keeps per class the first visited minimum of pow(f32 difference, 2) summed in double, below
// nearest_feature_dist.  The cloud is sorted by ring, so the walks cover the targets [lo, hi) of the rings nn_walk_ring gives, and the result is
// the arg-min over (distance, visiting rank) of every class: any evaluation order gives it.  nn_walk_d2 of the three gaps to a box is a lower
// bound of it for every point of the box (nn_gap <= |f32 difference|, exact conversion, monotone squares and sums).
NN_RULE_FN double nn_walk_d2(float dx, float dy, float dz) {
  const double ex = (double)dx, ey = (double)dy, ez = (double)dz;
  return ex * ex + ey * ey + ez * ez;
}
// rings of the window, clamped to the sensor's NS rings (a ring is int(intensity), :347,:436)
// (offset -ring_window: the first ring of the window, +ring_window: the last, 0: closest's own)
NN_RULE_FN int nn_walk_ring(int ring, int offset, int NS) { return nn_clampi(ring + offset, 0, NS - 1); }
// position of target k != closest in the reference's visiting order, for walks that stay inside [lo, hi)
NN_RULE_FN int nn_walk_rank(int k, int closest, int hi) { return k > closest ? k - closest - 1 : (hi - closest - 1) + (closest - 1 - k); }
// the class a candidate competes in: surf (kind 0): its second point is on closest's ring (:355), its third on another (:363); corner (kind 1): its
// second point is on another ring — strictly above going up, strictly below going down (:446,:462), which in a ring-sorted cloud is "another"
NN_RULE_FN bool nn_walk_second(int kind, bool same_ring) { return kind == 0 ? same_ring : !same_ring; }
NN_RULE_FN bool nn_walk_third(int kind, bool same_ring) { return kind == 0 && !same_ring; }
NN_RULE_FN bool nn_walk_better(double d, int rank, double bd, int brank) { return d < bd || (d == bd && rank < brank); }
// a row is a correspondence when the walk found its points (:397,:472)
NN_RULE_FN bool nn_lo_row_ok(int kind, int idx2, int idx3) { return kind == 0 ? (idx2 >= 0 && idx3 >= 0) : (idx2 >= 0); }

#endif
