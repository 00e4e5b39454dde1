// occ_math.h — the rule of the occupancy grid (alego_occ_*), shared by the kernels (kernels_occ.hip) and the host twins
// (alego_occ_ray_host, alego_occ_integrate_host, alego_occ_classify_host; alego_occ_mark_host of the static map, section 25): one definition, so the two cannot drift apart.  Plain C++ that a
// host compiler reads without the HIP runtime; no contraction (-ffp-contract=off).  The rule is the project's own.
//
// GRID: origin[3] is the world position of the corner of cell (0, 0, 0), cell[3] > 0 the edge lengths, n[3] >= 1 the cells per axis
// (n[0] n[1] n[2] <= 2^31 - 1); the linear index is (z n[1] + y) n[0] + x.
// RAY (o, e): o = the key pose's translation, e = the archived point under keypose_matrix / kf_transform (the f32 values map_gather writes),
// both widened to f64; everything after that is f64.
//   cell of a point   c_k = floor((x_k - origin_k) / cell_k): a point on a boundary belongs to the upper cell
//   bad               a non-finite coordinate, or |(x_k - origin_k) / cell_k| > 2^30 at either end: skipped
//   short             len2 = (dx dx + dy dy) + dz dz < min_range^2: skipped
//   truncated         max_range > 0 and len2 > max_range^2: e <- o + (e - o) (max_range / sqrt(len2)); the ray carries no hit
//   culled            both end cells below 0, or both at or beyond n_k, on some axis: skipped (the cell index is monotone along the ray)
// The tests are made in this order and a skipped ray is counted once, under the first that applies; a truncated ray that is culled
// afterwards counts as both.
// TRAVERSAL: rem_k = |c1_k - c0_k|, s_k the sign of the step, inv_k = 1 / (e_k - o_k) for axes with rem_k > 0.  The j-th crossing of axis k
// lies at boundary index i = c0_k + (s_k > 0 ? j + 1 : -j), position b = origin_k + i cell_k, parameter t_k(j) = (b - o_k) inv_k: a closed
// form in (ray, k, j), monotone in j under rounding (each operation is).  Each step takes the axis with the smallest t_k(j_k) among those
// with j_k < rem_k, ties to the lowest k.  So the walk is the merge of three sorted lists under the strict order (t, k, j): it visits
// 1 + sum rem_k cells and ends in the end cell whatever rounding does to t, the position of a crossing in it (occ_rank) and the state
// after m steps (occ_seek) follow from binary searches, and any lane can walk any piece of a ray.
// COUNTS: every visited cell but the last gets passes += 1, the last hits += 1 (passes += 1 for a truncated ray); cells inside the grid only.
// CLASSES: occupied (100) iff hits >= min_hits and (int64) hits hit_weight >= (int64) passes pass_weight; else 0 if passes > 0; else -1.
#ifndef ALEGO_OCC_MATH_H_
#define ALEGO_OCC_MATH_H_
#include <math.h>
#include <stdint.h>

#include "../../include/alego_mi355x.h"

#if defined(__HIPCC__)
#define OCC_FN __host__ __device__ inline
#else
#define OCC_FN inline
#endif

#define OCC_COORD_MAX 1073741824.0   // 2^30: cells beyond it (in units of the cell, from the origin) make a ray bad

// the options as the rule reads them: the squares of the ranges are formed once, on the host
struct OccGrid { double origin[3], cell[3]; int32_t n[3]; int32_t pad; double min_r2, max_range, max_r2; };
// a ray that is cast: start / end cell, step signs, crossings per axis and in all
struct OccRay { double o[3], inv[3]; int64_t rem[3], total; int32_t c0[3], c1[3], s[3], truncated; };
// the walk's state: crossings made per axis, the parameter of each axis's next crossing (unused where j == rem), the current cell
struct OccWalk { int64_t j[3]; double t[3]; int32_t c[3]; };

OCC_FN bool occ_finite(double x) { return x - x == 0.0; }

// nullptr when the options describe a grid, else why they do not
inline const char* occ_opts_fault(const alego_occ_opts* o) {
  for (int k = 0; k < 3; ++k) {
    if (!occ_finite(o->cell[k]) || !(o->cell[k] > 0.0)) return "cell must be positive and finite";
    if (!occ_finite(o->origin[k])) return "origin is not finite";
    if (o->n[k] < 1) return "n must be at least 1 on every axis";
  }
  if ((int64_t)o->n[0] * o->n[1] > 2147483647LL || (int64_t)o->n[0] * o->n[1] * o->n[2] > 2147483647LL) return "more than 2^31 - 1 cells";
  if (!occ_finite(o->min_range) || !occ_finite(o->max_range)) return "a range is not finite";
  if (o->min_range < 0.0) return "min_range is negative";
  return nullptr;
}
inline OccGrid occ_grid(const alego_occ_opts* o) {
  OccGrid G;
  for (int k = 0; k < 3; ++k) { G.origin[k] = o->origin[k]; G.cell[k] = o->cell[k]; G.n[k] = o->n[k]; }
  G.pad = 0;
  G.min_r2 = o->min_range * o->min_range; G.max_range = o->max_range; G.max_r2 = o->max_range * o->max_range;
  return G;
}
inline const char* occ_rule_fault(const alego_occ_rule* r) { return (r->min_hits < 0 || r->hit_weight < 0 || r->pass_weight < 0) ? "min_hits and the weights must not be negative" : nullptr; }

OCC_FN size_t occ_cells(const OccGrid& G) { return (size_t)G.n[0] * G.n[1] * G.n[2]; }
OCC_FN bool occ_inside(const OccGrid& G, const int32_t* c) { return c[0] >= 0 && c[0] < G.n[0] && c[1] >= 0 && c[1] < G.n[1] && c[2] >= 0 && c[2] < G.n[2]; }
OCC_FN size_t occ_index(const OccGrid& G, const int32_t* c) { return ((size_t)c[2] * G.n[1] + c[1]) * G.n[0] + c[0]; }
// (x - origin) / cell of one coordinate; its floor is the cell
OCC_FN double occ_coord(const OccGrid& G, int k, double x) { return (x - G.origin[k]) / G.cell[k]; }

// 0: the ray is cast, *R is complete; ALEGO_OCC_SKIP_*: it is skipped (R->truncated is valid either way)
OCC_FN int occ_ray_setup(const OccGrid& G, const float* of, const float* ef, OccRay* R) {
  double e[3], d[3], q0[3], q1[3];
  R->truncated = 0;
  for (int k = 0; k < 3; ++k) {
    R->o[k] = (double)of[k]; e[k] = (double)ef[k];
    if (!occ_finite(R->o[k]) || !occ_finite(e[k])) return ALEGO_OCC_SKIP_BAD;
  }
  for (int k = 0; k < 3; ++k) {
    q0[k] = occ_coord(G, k, R->o[k]); q1[k] = occ_coord(G, k, e[k]);
    if (!(fabs(q0[k]) <= OCC_COORD_MAX) || !(fabs(q1[k]) <= OCC_COORD_MAX)) return ALEGO_OCC_SKIP_BAD;
    d[k] = e[k] - R->o[k];
  }
  const double len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  if (len2 < G.min_r2) return ALEGO_OCC_SKIP_SHORT;
  if (G.max_range > 0.0 && len2 > G.max_r2) {
    const double f = G.max_range / sqrt(len2);
    for (int k = 0; k < 3; ++k) { e[k] = R->o[k] + d[k] * f; q1[k] = occ_coord(G, k, e[k]); }
    R->truncated = 1;
  }
  bool culled = false;
  R->total = 0;
  for (int k = 0; k < 3; ++k) {
    const int32_t c0 = (int32_t)floor(q0[k]), c1 = (int32_t)floor(q1[k]);
    R->c0[k] = c0; R->c1[k] = c1;
    culled = culled || (c0 < 0 && c1 < 0) || (c0 >= G.n[k] && c1 >= G.n[k]);
    R->s[k] = c1 > c0 ? 1 : (c1 < c0 ? -1 : 0);
    R->rem[k] = c1 > c0 ? (int64_t)c1 - c0 : (int64_t)c0 - c1;
    R->inv[k] = R->rem[k] > 0 ? 1.0 / (e[k] - R->o[k]) : 0.0;
    R->total += R->rem[k];
  }
  return culled ? ALEGO_OCC_SKIP_CULLED : 0;
}

// parameter of the j-th crossing of axis k (rem_k > 0, 0 <= j < rem_k)
OCC_FN double occ_t(const OccGrid& G, const OccRay& R, int k, int64_t j) {
  const int64_t i = (int64_t)R.c0[k] + (R.s[k] > 0 ? j + 1 : -j);
  const double b = G.origin[k] + (double)i * G.cell[k];
  return (b - R.o[k]) * R.inv[k];
}
// the walk after the crossings j[3] (their sum = the steps made)
OCC_FN void occ_walk_at(const OccGrid& G, const OccRay& R, const int64_t* j, OccWalk* W) {
  for (int k = 0; k < 3; ++k) {
    W->j[k] = j[k];
    W->c[k] = (int32_t)((int64_t)R.c0[k] + R.s[k] * j[k]);
    W->t[k] = j[k] < R.rem[k] ? occ_t(G, R, k, j[k]) : 0.0;
  }
}
OCC_FN void occ_walk_begin(const OccGrid& G, const OccRay& R, OccWalk* W) { const int64_t j[3] = {0, 0, 0}; occ_walk_at(G, R, j, W); }
// one step (the caller knows that one is left): the axis with the smallest parameter among those with crossings left, ties to the lowest axis
OCC_FN int occ_step(const OccGrid& G, const OccRay& R, OccWalk* W) {
  int a = -1;
  double ta = 0.0;
  for (int k = 0; k < 3; ++k)
    if (W->j[k] < R.rem[k] && (a < 0 || W->t[k] < ta)) { a = k; ta = W->t[k]; }
  for (int k = 0; k < 3; ++k)   // (the axis by comparison, not by index: the state stays in registers on the device)
    if (k == a) { W->j[k] += 1; W->c[k] += R.s[k]; if (W->j[k] < R.rem[k]) W->t[k] = occ_t(G, R, k, W->j[k]); }
  return a;
}

// crossings of axis k that the walk makes before a crossing of axis a with parameter t (k != a)
OCC_FN int64_t occ_before(const OccGrid& G, const OccRay& R, int k, int a, double t) {
  int64_t lo = 0, hi = R.rem[k];   // the crossings j < lo come before, those >= hi do not
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const double tk = occ_t(G, R, k, mid);
    if (tk < t || (tk == t && k < a)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// steps the walk makes before the j-th crossing of axis a: the cell index along the ray is rank + 1 behind that crossing
OCC_FN int64_t occ_rank(const OccGrid& G, const OccRay& R, int a, int64_t j) {
  const double t = occ_t(G, R, a, j);
  int64_t r = j;
  for (int k = 0; k < 3; ++k) if (k != a && R.rem[k] > 0) r += occ_before(G, R, k, a, t);
  return r;
}
// the crossings per axis after m steps (0 <= m <= total), from the closed form alone
OCC_FN void occ_seek(const OccGrid& G, const OccRay& R, int64_t m, int64_t* j) {
  for (int a = 0; a < 3; ++a) {
    int64_t lo = 0, hi = R.rem[a];
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (occ_rank(G, R, a, mid) < m) lo = mid + 1; else hi = mid;
    }
    j[a] = lo;
  }
}
// The cells of the ray inside the grid are those at steps [*m_in, *m_out] (the index is monotone on every axis, so they are one run); false: none
OCC_FN bool occ_clip(const OccGrid& G, const OccRay& R, int64_t* m_in, int64_t* m_out) {
  int64_t in = 0, out = R.total;
  for (int a = 0; a < 3; ++a) {
    // cell = c0 + s j, j in [0, rem]: inside for j in [lo, hi]
    const int64_t c0 = R.c0[a], n = G.n[a];
    int64_t lo, hi;
    if (R.s[a] >= 0) { lo = c0 < 0 ? -c0 : 0; hi = n - 1 - c0; }
    else { lo = c0 > n - 1 ? c0 - (n - 1) : 0; hi = c0; }
    if (hi > R.rem[a]) hi = R.rem[a];
    if (lo > hi) return false;
    const int64_t first = lo == 0 ? 0 : occ_rank(G, R, a, lo - 1) + 1;
    const int64_t last = hi >= R.rem[a] ? R.total : occ_rank(G, R, a, hi);
    if (first > in) in = first;
    if (last < out) out = last;
  }
  *m_in = in; *m_out = out;
  return in <= out;
}

// ---- classes ----
OCC_FN int8_t occ_class(const alego_occ_rule& r, uint32_t hits, uint32_t passes) {
  if ((int64_t)hits >= (int64_t)r.min_hits && (int64_t)hits * r.hit_weight >= (int64_t)passes * r.pass_weight) return 100;
  return passes > 0 ? 0 : -1;
}
// a column's class from its layers': 100 if any is 100, else 0 if any is 0, else -1
OCC_FN int8_t occ_class_merge(int8_t column, int8_t layer) { return column == 100 || layer == 100 ? 100 : (column == 0 || layer == 0 ? 0 : -1); }

// ---- the static map (alego_occ_mark, alego_map_assemble_static, alego_occ_mark_host) ----
// A point of the archive is judged by its own cell: e = the f32 world position map_gather writes, widened to f64, c_k = floor(occ_coord(G, k, e_k)),
// the expression that gives c1 in occ_ray_setup.  The tests in order: OUTSIDE (a non-finite coordinate, |q_k| > 2^30, a cell outside the grid),
// BELOW (use_keep_below and sensor_z < keep_below), OCCUPIED (class 100), UNKNOWN (class -1), NEIGHBOUR (class 0, protect_radius r > 0 and a cell
// of the grid within Chebyshev distance r of class 100), REMOVED (class 0 otherwise).  Only REMOVED points leave the map.
inline const char* occ_static_rule_fault(const alego_static_rule* r) {
  if (const char* why = occ_rule_fault(&r->occ)) return why;
  if (r->protect_radius < 0 || r->protect_radius > 2) return "protect_radius must lie in [0, 2]";
  if (r->use_keep_below && !occ_finite((double)r->keep_below)) return "keep_below is not finite";
  return nullptr;
}
inline alego_static_rule occ_static_rule_default() { return alego_static_rule{{1, 2, 1, 0}, 0, 0, 0.f, 0}; }
// hits / passes: the grid's counts (read only at cells inside the grid)
OCC_FN uint8_t occ_static_verdict(const OccGrid& G, const alego_static_rule& r, const uint32_t* hits, const uint32_t* passes, const float* ef, float sensor_z) {
  int32_t c[3];
  for (int k = 0; k < 3; ++k) {
    const double x = (double)ef[k];
    if (!occ_finite(x)) return ALEGO_STATIC_OUTSIDE;
    const double q = occ_coord(G, k, x);
    if (!(fabs(q) <= OCC_COORD_MAX)) return ALEGO_STATIC_OUTSIDE;
    c[k] = (int32_t)floor(q);
  }
  if (!occ_inside(G, c)) return ALEGO_STATIC_OUTSIDE;
  if (r.use_keep_below && sensor_z < r.keep_below) return ALEGO_STATIC_BELOW;
  const size_t i = occ_index(G, c);
  const int8_t cls = occ_class(r.occ, hits[i], passes[i]);
  if (cls == 100) return ALEGO_STATIC_OCCUPIED;
  if (cls < 0) return ALEGO_STATIC_UNKNOWN;
  const int32_t rad = r.protect_radius < 2 ? r.protect_radius : 2;   // (the host refuses more: a bound the loops can rely on)
  if (rad > 0) {
    int32_t lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = c[k] - rad < 0 ? 0 : c[k] - rad; hi[k] = c[k] + rad > G.n[k] - 1 ? G.n[k] - 1 : c[k] + rad; }
    int32_t d[3];
    for (d[2] = lo[2]; d[2] <= hi[2]; ++d[2])
      for (d[1] = lo[1]; d[1] <= hi[1]; ++d[1])
        for (d[0] = lo[0]; d[0] <= hi[0]; ++d[0]) {
          const size_t j = occ_index(G, d);
          if (occ_class(r.occ, hits[j], passes[j]) == 100) return ALEGO_STATIC_NEIGHBOUR;
        }
  }
  return ALEGO_STATIC_REMOVED;
}
inline void occ_mark_host(const OccGrid& G, const alego_static_rule& r, const uint32_t* hits, const uint32_t* passes, const alego_point* pts, const float* sensor_z,
                          int32_t n, uint8_t* verdict, int64_t* stats /* [ALEGO_STATIC_VERDICTS] */) {
  for (int32_t i = 0; i < n; ++i) {
    const float e[3] = {pts[i].x, pts[i].y, pts[i].z};
    const uint8_t v = occ_static_verdict(G, r, hits, passes, e, sensor_z ? sensor_z[i] : 0.f);
    verdict[i] = v;
    stats[v] += 1;
  }
}

// ---- the host twins ----
// The visited cells of one ray in order, the first `cap` of them to cells3[3 i + k]; *hit = 1 when the last cell takes a hit.  Returns the cells visited or a skip code.
inline int64_t occ_ray_host(const OccGrid& G, const float* o, const float* e, int32_t* cells3, int64_t cap, int32_t* hit) {
  OccRay R;
  if (const int r = occ_ray_setup(G, o, e, &R)) return r;
  OccWalk W;
  occ_walk_begin(G, R, &W);
  for (int64_t m = 0; m <= R.total; ++m) {
    if (m < cap && cells3) for (int k = 0; k < 3; ++k) cells3[3 * m + k] = W.c[k];
    if (m < R.total) occ_step(G, R, &W);
  }
  if (hit) *hit = R.truncated ? 0 : 1;
  return R.total + 1;
}
// one ray added into hits / passes (each may be null) and stats: the plain walk, every cell tested against the grid
inline void occ_add_host(const OccGrid& G, const float* o, const float* e, uint32_t* hits, uint32_t* passes, int64_t* stats) {
  OccRay R;
  stats[ALEGO_OCC_RAYS] += 1;
  const int r = occ_ray_setup(G, o, e, &R);
  if (R.truncated) stats[ALEGO_OCC_TRUNCATED] += 1;
  if (r) { stats[r == ALEGO_OCC_SKIP_SHORT ? ALEGO_OCC_SHORT : (r == ALEGO_OCC_SKIP_CULLED ? ALEGO_OCC_CULLED : ALEGO_OCC_BAD)] += 1; return; }
  OccWalk W;
  occ_walk_begin(G, R, &W);
  for (int64_t m = 0; m <= R.total; ++m) {
    if (occ_inside(G, W.c)) {
      const size_t i = occ_index(G, W.c);
      if (m == R.total && !R.truncated) { if (hits) hits[i] += 1; } else if (passes) passes[i] += 1;
      stats[ALEGO_OCC_UPDATES] += 1;
    }
    if (m < R.total) occ_step(G, R, &W);
  }
}
inline void occ_classify_host(const OccGrid& G, const alego_occ_rule& rule, const uint32_t* hits, const uint32_t* passes, int collapse_z, int8_t* out) {
  const size_t layer = (size_t)G.n[0] * G.n[1];
  for (size_t i = 0; i < layer; ++i) {
    int8_t col = -1;
    for (int z = 0; z < G.n[2]; ++z) {
      const int8_t c = occ_class(rule, hits[z * layer + i], passes[z * layer + i]);
      if (collapse_z) col = occ_class_merge(col, c); else out[z * layer + i] = c;
    }
    if (collapse_z) out[i] = col;
  }
}
#endif
