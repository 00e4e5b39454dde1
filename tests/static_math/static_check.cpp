// static_check.cpp — the static-map rule of csrc/occ_math.h read by a host compiler alone (no HIP runtime), built with AddressSanitizer and UBSan by
// tests/test_static_math.py.  10^4 random points on small grids (1 to 4 cells per axis, so that every neighbourhood meets faces and corners; the
// count arrays are exactly as large as the grid, so a read outside them is an error the sanitizer reports) against the plain definition: the cell
// by floor, the class from 64-bit products, the neighbourhood by a loop over EVERY cell of the grid and its Chebyshev distance.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "occ_math.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (point %d)\n", __FILE__, __LINE__, #c, g_pt); return 1; } } while (0)
static int g_pt = -1;

static int plain_class(const alego_occ_rule& r, uint32_t h, uint32_t p) {
  const long long hh = h, pp = p;
  if (hh >= r.min_hits && hh * r.hit_weight >= pp * r.pass_weight) return 100;
  return pp > 0 ? 0 : -1;
}
static int plain_verdict(const alego_occ_opts& o, const alego_static_rule& r, const std::vector<uint32_t>& hits, const std::vector<uint32_t>& passes, const float* e, float sz) {
  long long c[3];
  for (int k = 0; k < 3; ++k) {
    const double x = e[k];
    if (std::isnan(x) || std::isinf(x)) return ALEGO_STATIC_OUTSIDE;
    const double q = (x - o.origin[k]) / o.cell[k];
    if (std::fabs(q) > 1073741824.0) return ALEGO_STATIC_OUTSIDE;
    c[k] = (long long)std::floor(q);
  }
  for (int k = 0; k < 3; ++k) if (c[k] < 0 || c[k] >= o.n[k]) return ALEGO_STATIC_OUTSIDE;
  if (r.use_keep_below && sz < r.keep_below) return ALEGO_STATIC_BELOW;
  const size_t i = (size_t)((c[2] * o.n[1] + c[1]) * o.n[0] + c[0]);
  const int cls = plain_class(r.occ, hits.at(i), passes.at(i));
  if (cls == 100) return ALEGO_STATIC_OCCUPIED;
  if (cls == -1) return ALEGO_STATIC_UNKNOWN;
  for (int z = 0; z < o.n[2]; ++z)
    for (int y = 0; y < o.n[1]; ++y)
      for (int x = 0; x < o.n[0]; ++x) {
        const long long d = std::max(std::max(std::llabs(x - c[0]), std::llabs(y - c[1])), std::llabs(z - c[2]));
        if (d <= r.protect_radius && plain_class(r.occ, hits.at((size_t)(z * o.n[1] + y) * o.n[0] + x), passes.at((size_t)(z * o.n[1] + y) * o.n[0] + x)) == 100)
          return ALEGO_STATIC_NEIGHBOUR;
      }
  return ALEGO_STATIC_REMOVED;
}

int main() {
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> U01(0.0, 1.0);
  const float wild[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 3.0e9f, -3.0e9f,
                        1.0e30f, -3.0e38f, 1.5e9f};
  long seen[ALEGO_STATIC_VERDICTS] = {0, 0, 0, 0, 0, 0};
  for (g_pt = 0; g_pt < 10000; ++g_pt) {
    alego_occ_opts o = {{-1.25, 0.5, 2.0}, {0.5, 0.25, 1.0}, {1, 1, 1}, 0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) o.n[k] = 1 + (int)(rng() % 4);
    CHECK(!occ_opts_fault(&o));
    const OccGrid G = occ_grid(&o);
    const size_t cells = occ_cells(G);
    // the arrays end with the grid: a neighbour read beyond a face is a heap overflow
    std::vector<uint32_t> hits(cells), passes(cells);
    for (size_t i = 0; i < cells; ++i) {
      const unsigned kind = (unsigned)(rng() % 8);
      hits[i] = kind < 2 ? 0u : (kind == 7 ? 4000000000u : (uint32_t)(rng() % 4));
      passes[i] = kind == 0 ? 0u : (kind == 7 ? 4000000000u - (uint32_t)(rng() % 2) : (uint32_t)(rng() % 9));
    }
    alego_static_rule r = occ_static_rule_default();
    r.protect_radius = (int32_t)(rng() % 3);
    if (g_pt % 3 == 0) { r.use_keep_below = 1; r.keep_below = -0.25f; }
    if (g_pt % 5 == 0) r.occ = alego_occ_rule{(int32_t)(rng() % 3), 1 + (int32_t)(rng() % 3), 1 + (int32_t)(rng() % 3), 0};
    if (g_pt % 7 == 0) r.occ = alego_occ_rule{1, 2147483647, 2147483647, 0};
    CHECK(!occ_static_rule_fault(&r));
    float e[3];
    for (int k = 0; k < 3; ++k) {
      // inside or a fifth of a cell around the grid; every fourth point on a cell boundary (the far face included)
      const double q = -0.2 + U01(rng) * (o.n[k] + 0.4);
      e[k] = (float)(o.origin[k] + o.cell[k] * (g_pt % 4 == 0 ? std::floor(q + 0.5) : q));
    }
    if (g_pt % 50 == 0) e[rng() % 3] = wild[rng() % (sizeof(wild) / sizeof(wild[0]))];
    const float sz = (float)(U01(rng) - 0.75);
    const int want = plain_verdict(o, r, hits, passes, e, sz);
    const int got = occ_static_verdict(G, r, hits.data(), passes.data(), e, sz);
    CHECK(got == want);
    // the loop over points gives the same and counts it
    const alego_point p = {e[0], e[1], e[2], 0.f};
    uint8_t v = 99;
    int64_t stats[ALEGO_STATIC_VERDICTS] = {0, 0, 0, 0, 0, 0};
    occ_mark_host(G, r, hits.data(), passes.data(), &p, r.use_keep_below ? &sz : nullptr, 1, &v, stats);
    CHECK(v == want && stats[want] == 1);
    seen[want] += 1;
  }
  g_pt = -1;
  for (int k = 0; k < ALEGO_STATIC_VERDICTS; ++k)
    if (seen[k] < 100) { std::printf("FAILED: the cases are thin: verdict %d seen %ld times\n", k, seen[k]); return 1; }
  // the refusals of the rule
  alego_static_rule r = occ_static_rule_default();
  CHECK(!occ_static_rule_fault(&r));
  r.protect_radius = 3; CHECK(occ_static_rule_fault(&r)); r.protect_radius = -1; CHECK(occ_static_rule_fault(&r)); r.protect_radius = 2; CHECK(!occ_static_rule_fault(&r));
  r.keep_below = std::numeric_limits<float>::quiet_NaN(); CHECK(!occ_static_rule_fault(&r)); r.use_keep_below = 1; CHECK(occ_static_rule_fault(&r));
  r.keep_below = 0.f; r.occ.pass_weight = -1; CHECK(occ_static_rule_fault(&r));
  std::printf("static ok: occupied %ld unknown %ld outside %ld below %ld neighbour %ld removed %ld\n", seen[0], seen[1], seen[2], seen[3], seen[4], seen[5]);
  return 0;
}
