// occ_math_check.cpp — csrc/occ_math.h read by a host compiler alone (no HIP runtime), built with AddressSanitizer and UBSan by
// tests/test_occ_math.py.  For 10^4 random rays: the walk starts in the start cell, ends in the end cell, has 1 + sum rem_k cells and moves one
// step on one axis at a time; any sub-range computed from the closed form (occ_seek + occ_walk_at) equals the same range of the whole walk -
// what permits cutting a ray into pieces; occ_rank is the position of every crossing; occ_clip names exactly the cells inside the grid; a
// culled ray has none.  Then the classes on both sides of each of their three comparisons.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "occ_math.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (ray %d)\n", __FILE__, __LINE__, #c, g_ray); return 1; } } while (0)
static int g_ray = -1;

static int check_ray(const OccGrid& G, const float* o, const float* e, std::mt19937_64& rng, long* counts) {
  OccRay R;
  const int code = occ_ray_setup(G, o, e, &R);
  if (code == ALEGO_OCC_SKIP_SHORT || code == ALEGO_OCC_SKIP_BAD) { counts[1] += 1; return 0; }
  // (a culled ray is complete too: its walk must not touch the grid)
  std::vector<int32_t> cells;
  std::vector<int> axis;
  OccWalk W;
  occ_walk_begin(G, R, &W);
  for (int64_t m = 0; m <= R.total; ++m) {
    for (int k = 0; k < 3; ++k) cells.push_back(W.c[k]);
    if (m < R.total) axis.push_back(occ_step(G, R, &W));
  }
  const int64_t n = R.total + 1;
  CHECK(n == 1 + R.rem[0] + R.rem[1] + R.rem[2]);
  for (int k = 0; k < 3; ++k) { CHECK(cells[k] == R.c0[k]); CHECK(cells[3 * (n - 1) + k] == R.c1[k]); }
  int64_t seen[3] = {0, 0, 0};
  for (int64_t m = 0; m + 1 < n; ++m) {
    int moved = 0;
    for (int k = 0; k < 3; ++k) {
      const int d = cells[3 * (m + 1) + k] - cells[3 * m + k];
      if (d) { CHECK(d == R.s[k] && axis[m] == k); ++moved; }
    }
    CHECK(moved == 1);
    CHECK(occ_rank(G, R, axis[m], seen[axis[m]]) == m);   // the crossing's position from the closed form
    seen[axis[m]] += 1;
  }
  // sub-ranges from the closed form
  for (int rep = 0; rep < 4; ++rep) {
    const int64_t a = (int64_t)(rng() % (uint64_t)n), b = a + (int64_t)(rng() % (uint64_t)(n - a));
    int64_t j[3];
    occ_seek(G, R, a, j);
    CHECK(j[0] + j[1] + j[2] == a);
    OccWalk V;
    occ_walk_at(G, R, j, &V);
    for (int64_t m = a; m <= b; ++m) {
      for (int k = 0; k < 3; ++k) CHECK(V.c[k] == cells[3 * m + k]);
      if (m < R.total) CHECK(occ_step(G, R, &V) == axis[m]);
    }
  }
  // the clip against the plain test of every cell
  int64_t first = -1, last = -1, inside = 0;
  for (int64_t m = 0; m < n; ++m)
    if (occ_inside(G, &cells[3 * m])) { if (first < 0) first = m; last = m; ++inside; }
  int64_t m_in = 0, m_out = 0;
  const bool any = occ_clip(G, R, &m_in, &m_out);
  CHECK(any == (inside > 0));
  if (any) { CHECK(m_in == first && m_out == last && inside == last - first + 1); }
  if (code == ALEGO_OCC_SKIP_CULLED) { CHECK(inside == 0); counts[2] += 1; }
  counts[0] += 1; counts[3] += inside; counts[4] += n;
  return 0;
}

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> N01(0.0, 1.0);
  std::uniform_real_distribution<double> U01(0.0, 1.0);
  alego_occ_opts opts = {{-20.0, -20.0, -2.0}, {0.4, 0.4, 0.5}, {100, 100, 8}, 0, 0.0, 0.0};
  if (occ_opts_fault(&opts)) { std::printf("FAILED: the options\n"); return 1; }
  long counts[5] = {0, 0, 0, 0, 0};
  for (g_ray = 0; g_ray < 10000; ++g_ray) {
    if (g_ray == 5000) { opts.min_range = 1.0; opts.max_range = 25.0; }   // the second half: short and truncated rays too
    if (g_ray == 8000) { opts.n[0] = 30; opts.n[1] = 7; opts.n[2] = 1; opts.origin[0] = 3.0; }   // a grid most sensors lie outside of
    const OccGrid G = occ_grid(&opts);
    float o[3], e[3];
    double d[3], len = 0.0;
    for (int k = 0; k < 3; ++k) { o[k] = (float)(N01(rng) * (k == 2 ? 0.3 : 5.0)); d[k] = N01(rng) * (k == 2 ? 0.2 : 1.0); len += d[k] * d[k]; }
    const double range = 0.5 + 39.5 * U01(rng);
    for (int k = 0; k < 3; ++k) e[k] = (float)((double)o[k] + d[k] / std::sqrt(len) * range);
    if (g_ray % 10 == 0) for (int k = 0; k < 3; ++k) {   // every tenth ray starts and ends on cell boundaries: ties everywhere
      o[k] = (float)(opts.origin[k] + opts.cell[k] * std::floor(((double)o[k] - opts.origin[k]) / opts.cell[k]));
      e[k] = (float)(opts.origin[k] + opts.cell[k] * std::floor(((double)e[k] - opts.origin[k]) / opts.cell[k]));
    }
    if (check_ray(G, o, e, rng, counts)) return 1;
  }
  g_ray = -1;
  if (counts[0] < 8000 || counts[2] < 100 || counts[3] < 100000) { std::printf("FAILED: the cases are thin: %ld %ld %ld %ld\n", counts[0], counts[1], counts[2], counts[3]); return 1; }
  // classes: each comparison on both sides
  const alego_occ_rule r = {2, 2, 1, 0};
  CHECK(occ_class(r, 2, 0) == 100 && occ_class(r, 1, 0) == -1);           // hits >= min_hits
  CHECK(occ_class(r, 2, 4) == 100 && occ_class(r, 2, 5) == 0);            // hits * hit_weight >= passes * pass_weight
  CHECK(occ_class(r, 1, 1) == 0 && occ_class(r, 0, 0) == -1);             // passes > 0
  const alego_occ_rule big = {1, 2147483647, 2147483647, 0};              // (the products need 64 bits)
  CHECK(occ_class(big, 4000000000u, 4000000000u) == 100 && occ_class(big, 3999999999u, 4000000000u) == 0);
  CHECK(occ_class_merge(-1, -1) == -1 && occ_class_merge(-1, 0) == 0 && occ_class_merge(0, -1) == 0 && occ_class_merge(0, 100) == 100 && occ_class_merge(100, -1) == 100);
  std::printf("occ_math ok: %ld rays walked (%ld skipped, %ld culled), %ld cells, %ld inside\n", counts[0], counts[1], counts[2], counts[4], counts[3]);
  return 0;
}
