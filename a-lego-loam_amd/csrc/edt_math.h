// edt_math.h — the rule of the clearance field and the inflated cost map of the occupancy grid (alego_occ_distance, alego_occ_costmap; DESIGN.md
// section 26), shared by the kernels (kernels_edt.hip) and the host twins (alego_occ_distance_host, alego_occ_cost_table_host,
// alego_occ_costmap_host): one definition, so the two cannot drift apart.  Plain C++ that a host compiler reads without the HIP runtime.
//
// DOMAIN: the class array alego_occ_classify gives: n[0] n[1] n[2] cells, or n[0] n[1] 1 with collapse_z; linear index (z n[1] + y) n[0] + x.  An
// axis with one cell contributes no displacement.  Every axis with more than one cell must have the same edge length s (doubles, compared for
// equality); with no such axis s = cell[0].  The sum of (n_k - 1)^2 over the axes must not exceed 2^32 - 2: no finite value reaches FAR.
// SOURCES: the cells of class 100; with unknown_is_obstacle those of class -1 as well.
// SQUARED DISTANCE: d2(c) = min over the sources c' of dx^2 + dy^2 + dz^2 in cells, u32; EDT_FAR where there is no source.  max_cells = r > 0
// turns every d2 > r^2 into FAR (applied at the end); r = 0: no limit; 0 <= r <= 65535.  The metric distance is s sqrt(d2).
// ALGORITHM: separable and exact in integers.  Pass X: per (y, z) line the distance g to the nearest source along x, stored as g^2.  Passes Y and
// Z: h(u) = min over i of f(i) + (u - i)^2 along the axis, by the lower envelope of the parabolas (Meijster's two sweeps, edt_envelope);
// lines without a finite value contribute no parabola.  The work per cell is bounded whatever the scene: every cell is pushed and popped at
// most once per pass.
// COST: costmap_2d's computeCost as a table over d2 (edt_cost_table); the cost of a cell is edt_cost.
#ifndef ALEGO_EDT_MATH_H_
#define ALEGO_EDT_MATH_H_
#include <math.h>
#include <stdint.h>

#include "../../include/alego_mi355x.h"

#if defined(__HIPCC__)
#define EDT_FN __host__ __device__ inline
#else
#define EDT_FN inline
#endif

#define EDT_FAR 0xFFFFFFFFu
#define EDT_MAX_CELLS 65535        // the largest cap
#define EDT_SUM_MAX 4294967294LL   // 2^32 - 2: the largest sum of (n_k - 1)^2
#define EDT_TABLE_R_MAX 4095       // the largest inflation radius in cells

static_assert(EDT_FAR == ALEGO_OCC_FAR, "one value for a cell without a source");

EDT_FN bool edt_finite(double x) { return x - x == 0.0; }

// ---- the domain ----
// nullptr when (n, cap) describe a domain, else why they do not
inline const char* edt_dims_fault(const int32_t* n, int32_t max_cells) {
  int64_t sum = 0;
  for (int k = 0; k < 3; ++k) {
    if (n[k] < 1) return "n must be at least 1 on every axis";
    sum += (int64_t)(n[k] - 1) * (n[k] - 1);   // (n_k <= 2^31 - 1: each square is below 2^62)
    if (sum > EDT_SUM_MAX) return "the squared diagonal of the grid exceeds 2^32 - 2 cells";
  }
  if ((int64_t)n[0] * n[1] > 2147483647LL || (int64_t)n[0] * n[1] * n[2] > 2147483647LL) return "more than 2^31 - 1 cells";
  if (max_cells < 0 || max_cells > EDT_MAX_CELLS) return "max_cells must lie in [0, 65535]";
  return nullptr;
}
// the domain of a grid (cells per axis, edge lengths): dom[3] and *s; nullptr, or why the grid has none
inline const char* edt_domain(const int32_t* n, const double* cell, int collapse_z, int32_t* dom, double* s) {
  dom[0] = n[0]; dom[1] = n[1]; dom[2] = collapse_z ? 1 : n[2];
  bool have = false;
  *s = cell[0];
  for (int k = 0; k < 3; ++k) {
    if (dom[k] <= 1) continue;
    if (!have) { *s = cell[k]; have = true; }
    else if (!(cell[k] == *s)) return "the axes with more than one cell must have one edge length";
  }
  return nullptr;
}

EDT_FN bool edt_source(int8_t cls, int unknown_is_obstacle) { return cls == 100 || (unknown_is_obstacle && cls < 0); }

// ---- pass X ----
// g^2 of a cell at x whose nearest sources along the line are at `left` <= x (-1: none) and `right` >= x (n: none)
EDT_FN uint32_t edt_g2(int32_t x, int32_t left, int32_t right, int32_t n) {
  uint32_t g = 0xFFFFFFFFu;
  if (left >= 0) g = (uint32_t)(x - left);
  if (right < n && (uint32_t)(right - x) < g) g = (uint32_t)(right - x);
  return g == 0xFFFFFFFFu ? EDT_FAR : g * g;   // (g <= 65535 by edt_dims_fault)
}

// ---- passes Y and Z: the lower envelope of one line ----
// value of the parabola of cell i (f(i) = fi, finite) at u
EDT_FN int64_t edt_parabola(int32_t u, int32_t i, uint32_t fi) { const uint32_t d = (uint32_t)(u > i ? u - i : i - u); return (int64_t)((uint64_t)d * d) + (int64_t)fi; }
// numerator of sep: non-negative after the pop loop, since then parabola(t, i) <= parabola(t, u) for the t >= 0 where i starts
// (u u - i i + f(u) - f(i), with u u - i i as one 32 x 32 -> 64 bit product: 0 <= i < u <= 65535)
EDT_FN int64_t edt_sep_num(int32_t i, uint32_t fi, int32_t u, uint32_t fu) { return (int64_t)((uint64_t)(uint32_t)(u - i) * (uint32_t)(u + i)) + (int64_t)fu - (int64_t)fi; }
// sep(i, u) = num div (2 (u - i)): the last cell at which the parabola of i (< u) is not above that of u.  The parabola of u starts at
// w = 1 + sep and joins the envelope only if w < n.  With h = num div 2 and k = u - i, sep = h div k; h >= k n means w > n, and otherwise
// h < k n <= 65535 * 65536 fits 32 bits: one 32-bit division, none of 64.  Returns w, or n where the parabola does not join.
EDT_FN int32_t edt_start(int64_t num, int32_t i, int32_t u, int32_t n) {
  const uint64_t h = (uint64_t)num >> 1;
  const uint32_t k = (uint32_t)(u - i);
  if (h >= (uint64_t)k * (uint32_t)n) return n;
  const uint32_t w = 1u + (uint32_t)h / k;
  return w < (uint32_t)n ? (int32_t)w : n;
}

// A parabola of the envelope: its cell, where it starts, and its value f(cell)
struct EdtTop { int32_t i, t; uint32_t f; };
#define EDT_AHEAD 8   // cells whose values are fetched before the block in front of them is worked through

// One line of n <= 65536 cells.  f(u): the input (EDT_FAR: none); out(u, v): receives v = the minimum as int64, or -1 where the line has no
// finite value; st: the stack of the envelope's parabolas, st.put(q, top) / st.get(q) for 0 <= q < n.  check(num): called with every sep
// numerator (the host check asserts num >= 0).  No step waits for memory it could have asked for earlier: f is read once per cell, EDT_AHEAD
// cells ahead of the pops; the two upper entries of the stack are kept in registers, so a pop uses what is there and fetches the entry that
// comes next (a push fetches nothing), and an entry carries its f.
template <class Load, class Store, class Stack, class Check>
EDT_FN void edt_envelope(int32_t n, Load f, Store out, Stack st, Check check) {
  int32_t q = -1;
  EdtTop top = {0, 0, 0}, below = {0, 0, 0};   // entries q and q - 1 (below: valid while q >= 1)
  uint32_t cur[EDT_AHEAD], nxt[EDT_AHEAD];
#pragma unroll
  for (int k = 0; k < EDT_AHEAD; ++k) nxt[k] = k < n ? f(k) : EDT_FAR;
  for (int32_t u0 = 0; u0 < n; u0 += EDT_AHEAD) {
#pragma unroll
    for (int k = 0; k < EDT_AHEAD; ++k) cur[k] = nxt[k];
#pragma unroll
    for (int k = 0; k < EDT_AHEAD; ++k) { const int64_t v = (int64_t)u0 + EDT_AHEAD + k; nxt[k] = v < n ? f((int32_t)v) : EDT_FAR; }
#pragma unroll
    for (int k = 0; k < EDT_AHEAD; ++k) {
      const int32_t u = u0 + k;
      const uint32_t fu = cur[k];
      if (u >= n || fu == EDT_FAR) continue;
      while (q >= 0 && edt_parabola(top.t, top.i, top.f) > edt_parabola(top.t, u, fu)) {
        --q; top = below;
        if (q >= 1) below = st.get(q - 1);
      }
      if (q < 0) {
        q = 0; top = EdtTop{u, 0, fu};
        st.put(0, top);
      } else {
        const int64_t num = edt_sep_num(top.i, top.f, u, fu);
        check(num);
        const int32_t w = edt_start(num, top.i, u, n);
        if (w < n) {
          ++q; below = top; top = EdtTop{u, w, fu};
          st.put(q, top);
        }
      }
    }
  }
  for (int32_t u = n - 1; u >= 0; --u) {
    out(u, q < 0 ? (int64_t)-1 : edt_parabola(u, top.i, top.f));
    if (q >= 0 && u == top.t) {
      --q; top = below;
      if (q >= 1) below = st.get(q - 1);
    }
  }
}

// ---- the end: cap and statistics ----
EDT_FN uint32_t edt_cap(uint32_t d2, uint32_t r2 /* 0: no limit */) { return (r2 > 0 && d2 != EDT_FAR && d2 > r2) ? EDT_FAR : d2; }

// ---- the cost table (costmap_2d's computeCost over d2) ----
// nullptr, or why the parameters give no table; *r = ceil(inflation_radius / s)
inline const char* edt_inflation_fault(double s, const alego_occ_inflation* p, int32_t* r) {
  if (!edt_finite(s) || !(s > 0.0)) return "the cell's edge must be positive and finite";
  if (!edt_finite(p->inscribed_radius) || !edt_finite(p->inflation_radius) || !edt_finite(p->cost_scaling)) return "a radius or the scaling is not finite";
  if (p->inscribed_radius < 0.0 || p->inflation_radius < 0.0 || p->cost_scaling < 0.0) return "a radius or the scaling is negative";
  if (p->inflation_radius < p->inscribed_radius) return "inflation_radius is below inscribed_radius";
  const double rc = ceil(p->inflation_radius / s);
  if (!(rc <= (double)EDT_TABLE_R_MAX)) return "the inflation radius exceeds 4095 cells";
  *r = (int32_t)rc;
  return nullptr;
}
// table[0, r r]: the one function behind the twin and the device path
inline void edt_cost_table(double s, const alego_occ_inflation* p, int32_t r, uint8_t* table) {
  table[0] = 254;
  for (int64_t d2 = 1; d2 <= (int64_t)r * r; ++d2) {
    const double dist = sqrt((double)d2) * s;
    if (dist <= p->inscribed_radius) table[d2] = 253;
    else table[d2] = (uint8_t)(252.0 * exp(-p->cost_scaling * (dist - p->inscribed_radius)));
  }
}
// the cost of one cell: 254 on a source; else t = table[d2] (0 beyond the table or where d2 is FAR), kept by a free cell, and by an unknown one
// only from 1 (inflate_unknown) or 253 upwards, which is otherwise 255 (NO_INFORMATION)
EDT_FN uint8_t edt_cost(int8_t cls, uint32_t d2, int unknown_is_obstacle, const uint8_t* table, int32_t n_table, int inflate_unknown) {
  if (edt_source(cls, unknown_is_obstacle)) return 254;
  const uint8_t t = (d2 != EDT_FAR && d2 < (uint32_t)n_table) ? table[d2] : 0;
  if (cls >= 0) return t;
  return t >= (inflate_unknown ? 1 : 253) ? t : 255;
}

// ---- the host twins ----
struct EdtHostStack {
  EdtTop* e;
  void put(int32_t q, const EdtTop& v) const { e[q] = v; }
  EdtTop get(int32_t q) const { return e[q]; }
};
struct EdtNoCheck { EDT_FN void operator()(int64_t) const {} };

// d2[cells] (work[cells] and stack[max n_k] are scratch); stats[ALEGO_EDT_STATS] may be null.  The caller has passed edt_dims_fault.
inline void edt_distance_host(const int8_t* cls, const int32_t* n, int unknown_is_obstacle, int32_t max_cells, uint32_t* d2, uint32_t* work, EdtTop* stack,
                              int64_t* stats) {
  const int64_t n0 = n[0], n1 = n[1], n2 = n[2], layer = n0 * n1, cells = layer * n2;
  // pass X: two sweeps per line
  for (int64_t l = 0; l < n1 * n2; ++l) {
    const int8_t* c = cls + l * n0;
    uint32_t* o = d2 + l * n0;
    int32_t left = -1;
    for (int32_t x = 0; x < n0; ++x) { if (edt_source(c[x], unknown_is_obstacle)) left = x; o[x] = (uint32_t)left; }   // (the left source for now)
    int32_t right = (int32_t)n0;
    for (int32_t x = (int32_t)n0 - 1; x >= 0; --x) { if (edt_source(c[x], unknown_is_obstacle)) right = x; o[x] = edt_g2(x, (int32_t)o[x], right, (int32_t)n0); }
  }
  uint32_t *in = d2, *out = work;
  const EdtHostStack st{stack};
  for (int axis = 1; axis <= 2; ++axis) {
    const int64_t len = n[axis], inner = axis == 1 ? n0 : layer, lines = cells / len;
    if (len <= 1) continue;
    for (int64_t l = 0; l < lines; ++l) {
      const int64_t base = (l / inner) * (len * inner) + l % inner;
      const uint32_t* fi = in + base;
      uint32_t* fo = out + base;
      edt_envelope((int32_t)len, [=](int32_t u) { return fi[u * inner]; }, [=](int32_t u, int64_t v) { fo[u * inner] = v < 0 ? EDT_FAR : (uint32_t)v; }, st, EdtNoCheck());
    }
    uint32_t* t = in; in = out; out = t;
  }
  const uint32_t r2 = (uint32_t)max_cells * (uint32_t)max_cells;
  int64_t sources = 0, far = 0, max_d2 = -1;
  for (int64_t i = 0; i < cells; ++i) {
    const uint32_t v = edt_cap(in[i], r2);
    d2[i] = v;
    if (v == 0) ++sources;
    if (v == EDT_FAR) ++far; else if ((int64_t)v > max_d2) max_d2 = v;
  }
  if (stats) { stats[ALEGO_EDT_SOURCES] = sources; stats[ALEGO_EDT_FAR_CELLS] = far; stats[ALEGO_EDT_MAX_D2] = max_d2; }
}
#endif
