// Host check of csrc/vox_merge.h (and of the host-readable grid arithmetic of csrc/vgrid.h): the merge form (runs and ranks, as the kernel) of
// VoxelGrid(leaf)(S ++ O) and the rank-by-counting filter of a small cloud against a plain restatement of pcl::VoxelGrid —
// bounding box, leaf-too-small rule, box-relative voxel ids in int arithmetic that wraps, std::stable_sort of the concatenation
// by id, sums from 0.f in that order, divided by (float)count — compared bit for bit.  Built by tests/test_vox_merge.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "vox_merge.h"

typedef std::vector<float4> Cloud;
static float4 P(float x, float y, float z, float w = 1.f) { float4 p; p.x = x; p.y = y; p.z = z; p.w = w; return p; }
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// ---- the plain restatement -------------------------------------------------------------------------------------------------
struct PlainGrid { bool pass; int minb[3], divb[3]; double cells; };
static PlainGrid plain_grid(const Cloud& c, float leaf) {
  PlainGrid g;
  const float inv = 1.0f / leaf;
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (const float4& p : c) {
    const float v[3] = {p.x, p.y, p.z};
    for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], v[a]); mx[a] = std::max(mx[a], v[a]); }
  }
  const int64_t dx = (int64_t)((mx[0] - mn[0]) * inv) + 1, dy = (int64_t)((mx[1] - mn[1]) * inv) + 1, dz = (int64_t)((mx[2] - mn[2]) * inv) + 1;
  g.pass = dx * dy * dz > (int64_t)2147483647;
  for (int a = 0; a < 3; ++a) { g.minb[a] = (int)std::floor(mn[a] * inv); g.divb[a] = (int)std::floor(mx[a] * inv) - g.minb[a] + 1; }
  g.cells = (double)g.divb[0] * (double)g.divb[1] * (double)g.divb[2];
  return g;
}
static uint32_t plain_id(const PlainGrid& g, const float4& p, float inv) {
  const int i0 = (int)(std::floor(p.x * inv) - (float)g.minb[0]), i1 = (int)(std::floor(p.y * inv) - (float)g.minb[1]), i2 = (int)(std::floor(p.z * inv) - (float)g.minb[2]);
  return (uint32_t)i0 + (uint32_t)i1 * (uint32_t)g.divb[0] + (uint32_t)i2 * ((uint32_t)g.divb[0] * (uint32_t)g.divb[1]);
}
static Cloud plain_filter(const Cloud& c, float leaf) {
  if (c.empty()) return c;
  const PlainGrid g = plain_grid(c, leaf);
  if (g.pass) return c;
  const float inv = 1.0f / leaf;
  std::vector<std::pair<uint32_t, int>> o(c.size());
  for (size_t i = 0; i < c.size(); ++i) o[i] = {plain_id(g, c[i], inv), (int)i};
  std::stable_sort(o.begin(), o.end(), [](const std::pair<uint32_t, int>& a, const std::pair<uint32_t, int>& b) { return a.first < b.first; });
  Cloud out;
  for (size_t a = 0; a < o.size();) {
    size_t b = a;
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    for (; b < o.size() && o[b].first == o[a].first; ++b) { const float4& p = c[o[b].second]; sx += p.x; sy += p.y; sz += p.z; si += p.w; }
    const float fn = (float)(b - a);
    out.push_back(P(sx / fn, sy / fn, sz / fn, si / fn));
    a = b;
  }
  return out;
}
// what the merge may refuse, stated on the plain grid: S's cells (k, j, i) not in lexicographic order, too many O points, a cell outside
// -2^20 .. 2^20 - 1, the leaf-too-small rule, 2^32 cells or more
static bool plain_must_refuse(const Cloud& S, const Cloud& O, float leaf, int ocap) {
  const float inv = 1.0f / leaf;
  Cloud all = S;
  all.insert(all.end(), O.begin(), O.end());
  if (all.empty()) return false;
  if ((int)O.size() > ocap) return true;
  for (const float4& p : all) if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) return true;
  auto cell = [&](const float4& p, int a) { return (double)std::floor((a == 0 ? p.x : a == 1 ? p.y : p.z) * inv); };
  for (size_t i = 1; i < S.size(); ++i) {
    int cmp = 0;
    for (int a = 2; a >= 0 && cmp == 0; --a) cmp = cell(S[i - 1], a) < cell(S[i], a) ? -1 : (cell(S[i - 1], a) > cell(S[i], a) ? 1 : 0);
    if (cmp > 0) return true;
  }
  for (const float4& p : all) for (int a = 0; a < 3; ++a) if (cell(p, a) < -1048576.0 || cell(p, a) > 1048575.0) return true;
  const PlainGrid g = plain_grid(all, leaf);
  return g.pass || g.cells > 4294967295.0;
}

// ---- the header's forms, as lm_total_merge applies them ----------------------------------------------------------------------
static Cloud counted_filter(const Cloud& c, float leaf) {   // part a: a cloud of at most LT_OCAP points
  const int n = (int)c.size();
  if (n == 0) return c;
  const float inv = 1.0f / leaf;
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (const float4& p : c) vgr_box_add(mn, mx, p);
  if (vgr_leaf_too_small(mn, mx, inv)) return c;
  const VgrGeom g = vgr_geom(mn, mx, inv);
  std::vector<vm_u64> key(n), skey(n);
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) key[i] = vgr_id(g, c[i], inv);
  for (int i = 0; i < n; ++i) { const int r = vm_rank(key.data(), n, i); skey[r] = key[i]; idx[r] = i; }
  Cloud out;
  for (int m = 0; m < n; ++m) {
    if (m > 0 && skey[m] == skey[m - 1]) continue;
    int b = m + 1;
    while (b < n && skey[b] == skey[m]) ++b;
    out.push_back(vm_centroid([&](int j) { return c[idx[j]]; }, m, b));
  }
  return out;
}
static bool header_refuses(const Cloud& S, const Cloud& O, float leaf) {   // part b's decision, from the box, the order of S's keys and O's size
  const int ns = (int)S.size(), no = (int)O.size();
  if (ns + no == 0) return false;
  const float inv = 1.0f / leaf;
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  bool good = true;
  for (int i = 0; i < ns; ++i) { vgr_box_add(mn, mx, S[i]); good = good && vm_finite(S[i]); }
  for (int i = 0; i < no; ++i) { vgr_box_add(mn, mx, O[i]); good = good && vm_finite(O[i]); }
  if (good) for (int i = 1; i < ns; ++i) good = good && vkey_of(S[i - 1], inv) <= vkey_of(S[i], inv);
  return vm_refuse(good, no, mn, mx, inv);
}

// the form the kernel computes an accepted pair in, without the merged cloud: a voxel's run is an S run followed by the O elements of its key
// (vm_count_less / vm_count_le on O's sorted keys), its output rank the S heads and the O-only voxels before it
static Cloud ranked_filter(const Cloud& S, const Cloud& O, float leaf) {
  const int ns = (int)S.size(), no = (int)O.size();
  const float inv = 1.0f / leaf;
  std::vector<vm_u64> key(no), skey(no), ks(ns);
  std::vector<int> idx(no), hs(ns + 1, 0), oop(no + 1, 0), only(no, 0);
  for (int j = 0; j < no; ++j) key[j] = vkey_of(O[j], inv);
  for (int j = 0; j < no; ++j) { const int r = vm_rank(key.data(), no, j); skey[r] = key[j]; idx[r] = j; }
  for (int i = 0; i < ns; ++i) ks[i] = vkey_of(S[i], inv);
  for (int i = 0; i < ns; ++i) hs[i + 1] = hs[i] + ((i == 0 || ks[i - 1] != ks[i]) ? 1 : 0);
  for (int i = 0; i <= ns; ++i)   // the O elements strictly between two S keys (before the first, behind the last)
    for (int j = i == 0 ? 0 : vm_count_le(skey.data(), no, ks[i - 1]); j < (i == ns ? no : vm_count_less(skey.data(), no, ks[i])); ++j) only[j] = 1 + hs[i];
  for (int j = 0; j < no; ++j) oop[j + 1] = oop[j] + ((only[j] && (j == 0 || skey[j - 1] != skey[j])) ? 1 : 0);
  Cloud out(hs[ns] + oop[no], P(NAN, NAN, NAN, NAN));
  for (int i = 0; i < ns; ++i) {
    if (i > 0 && ks[i - 1] == ks[i]) continue;
    const int ol = vm_count_less(skey.data(), no, ks[i]), ole = vm_count_le(skey.data(), no, ks[i]);
    int nsr = 1;
    while (i + nsr < ns && ks[i + nsr] == ks[i]) ++nsr;
    out[hs[i] + oop[ol]] = vm_centroid([&](int q) { return q < nsr ? S[i + q] : O[idx[ol + q - nsr]]; }, 0, nsr + ole - ol);
  }
  for (int j = 0; j < no; ++j) {
    if (!only[j] || (j > 0 && skey[j - 1] == skey[j])) continue;
    int e = j + 1;
    while (e < no && skey[e] == skey[j]) ++e;
    out[only[j] - 1 + oop[j]] = vm_centroid([&](int q) { return O[idx[q]]; }, j, e);
  }
  return out;
}

static bool bit_equal(const Cloud& a, const Cloud& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float4)) == 0); }

// one S / O pair: the refusal is the plain statement's, an accepted pair equals the plain filter of the concatenation
static bool check_pair(const char* what, const Cloud& S, const Cloud& O, float leaf, int want_refused = -1, int want_vox = -1) {
  Cloud all = S;
  all.insert(all.end(), O.begin(), O.end());
  const bool refused = header_refuses(S, O, leaf);
  CHECK(refused == plain_must_refuse(S, O, leaf, LT_OCAP), "%s: refused %d", what, (int)refused);
  if (want_refused >= 0) CHECK((int)refused == want_refused, "%s: refused %d, wanted %d", what, (int)refused, want_refused);
  if (refused) return true;
  const Cloud want = plain_filter(all, leaf), ranked = ranked_filter(S, O, leaf);
  CHECK(bit_equal(ranked, want), "%s: %zu voxels vs %zu of the plain filter", what, ranked.size(), want.size());
  if (want_vox >= 0) CHECK((int)want.size() == want_vox, "%s: %zu voxels, the case was built for %d", what, want.size(), want_vox);
  return false;
}

int main() {
  const float LS = 0.8f, LO = 1.0f;
  std::mt19937 rng(20240519u);
  auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
  // ---- random pairs: S and O by the plain filter from raw clouds; half of the cases on a 0.05 m lattice, whose points sit on cell boundaries
  int refused = 0, cases = 0, multi = 0;
  for (int it = 0; it < 600; ++it) {
    const bool lattice = it % 2 == 1;
    const float ext = it % 3 == 0 ? 8.f : 40.f, leaf_o = it % 4 < 2 ? LO : LS;
    auto q = [&](float v) { return lattice ? 0.05f * std::floor(v * 20.f) : v; };
    Cloud rs, ro;
    const int nrs = (int)uni(0.f, it % 5 == 0 ? 40.f : 3000.f), nro = (int)uni(0.f, it % 7 == 0 ? 3.f : 120.f);
    for (int i = 0; i < nrs; ++i) rs.push_back(P(q(uni(-ext, ext)), q(uni(-ext, ext)), q(uni(-2.f, 3.f)), uni(0.f, 16.f)));
    for (int i = 0; i < nro; ++i) ro.push_back(P(q(uni(-ext, ext)), q(uni(-ext, ext)), q(uni(-2.f, 3.f)), uni(0.f, 16.f)));
    const Cloud S = plain_filter(rs, LS), O = plain_filter(ro, leaf_o);
    CHECK(bit_equal(counted_filter(ro.size() <= (size_t)LT_OCAP ? ro : Cloud(), leaf_o), ro.size() <= (size_t)LT_OCAP ? O : Cloud()), "random %d: the counted filter of O", it);
    multi += S.size() + O.size() > plain_filter([&] { Cloud a = S; a.insert(a.end(), O.begin(), O.end()); return a; }(), LS).size();
    refused += check_pair("random", S, O, LS);
    ++cases;
  }
  std::printf("random pairs: %d, refused %d (%.2f %%), with a voxel of several points %d\n", cases, refused, 100.0 * refused / cases, multi);
  CHECK(refused * 100 <= cases, "more than 1 %% of the random pairs were refused");
  CHECK(multi * 2 > cases, "the random pairs hardly ever share a voxel");

  // ---- the counted filter on its own: duplicates, one voxel, the capacity, the leaf-too-small rule
  for (int it = 0; it < 60; ++it) {
    Cloud c;
    const int n = it < 4 ? (it == 0 ? 1 : LT_OCAP - 2 + it) : (int)uni(1.f, 200.f);
    const float ext = it % 2 ? 3.f : 60.f;
    for (int i = 0; i < n; ++i) c.push_back(P(uni(-ext, ext), uni(-ext, ext), uni(-1.f, 1.f), (float)i));
    CHECK(bit_equal(counted_filter(c, LO), plain_filter(c, LO)), "counted filter, case %d", it);
  }
  { Cloud c = {P(-2000.f, -2000.f, -2000.f), P(2000.f, 2000.f, 2000.f), P(0.f, -0.f, 0.f)}; CHECK(plain_grid(c, LO).pass && bit_equal(counted_filter(c, LO), c), "counted filter past the leaf-too-small rule"); }

  // ---- built cases
  const float E1 = 5.5999994f, E2 = -1.6000001f;
  {   // a centroid that leaves its voxel: three equal points average into the next 0.8 m cell
    const float inv = 1.0f / LS;
    for (float e : {E1, E2, -E1, -E2}) {
      const Cloud S = plain_filter({P(e, 0.1f, 0.1f), P(e, 0.1f, 0.1f), P(e, 0.1f, 0.1f)}, LS);
      if (e == E1 || e == E2) CHECK(S.size() == 1 && std::floor(S[0].x * inv) == std::floor(e * inv) + 1.f, "premise: the centroid %.9g of three %.9g stays in its cell", S[0].x, e);
      check_pair("escape alone", S, {}, LS, 0, 1);
      check_pair("escape + outlier in the old cell", S, {P(e, 0.2f, 0.2f)}, LS, 0);
      check_pair("escape + outlier in the new cell", S, {P(S[0].x, 0.2f, 0.2f)}, LS, 0, 1);
    }
    // ... into an occupied neighbour: S holds two points of one cell, which merge
    Cloud S = plain_filter({P(E1, 0.1f, 0.1f), P(E1, 0.1f, 0.1f), P(E1, 0.1f, 0.1f), P(5.7f, 0.1f, 0.1f)}, LS);
    CHECK(S.size() == 2 && vkey_of(S[0], inv) == vkey_of(S[1], inv), "premise: the escaped centroid shares the neighbour's cell");
    check_pair("escape into an occupied neighbour", S, {}, LS, 0, 1);
    check_pair("escape into an occupied neighbour + outliers", S, {P(5.9f, 0.3f, 0.3f), P(5.0f, 0.3f, 0.3f)}, LS, 0, 2);
    // ... backwards in the order: the y cell grows past a later point of the old y cell
    S = plain_filter({P(3.0f, E1, 0.1f), P(3.0f, E1, 0.1f), P(3.0f, E1, 0.1f), P(5.0f, 5.0f, 0.1f)}, LS);
    CHECK(S.size() == 2 && vkey_of(S[0], inv) > vkey_of(S[1], inv), "premise: the escaped centroid breaks the order");
    check_pair("escape that breaks the order", S, {P(0.f, 0.f, 0.f)}, LS, 1);
    check_pair("a pass-through first round (S unsorted)", {P(5.f, 5.f, 5.f), P(0.f, 0.f, 0.f)}, {P(1.f, 1.f, 1.f)}, LS, 1);
  }
  {   // -0.f: a voxel of one point gives +0.f
    const Cloud S = {P(-0.f, -0.f, -0.f, -0.f), P(1.f, -0.f, 0.f)}, O = {P(-0.f, 3.f, -0.f), P(-0.f, 3.1f, 0.f)};
    check_pair("-0.f", S, O, LS, 0, 3);
    const Cloud out = ranked_filter(S, O, LS);
    uint32_t bits; std::memcpy(&bits, &out[0].x, 4);
    CHECK(bits == 0u, "-0.f alone in its voxel came out as %08x", bits);
  }
  {   // where O falls among S's keys
    Cloud S;
    for (int i = 0; i < 40; ++i) S.push_back(P(0.8f * (float)i + 0.3f, 0.3f, 0.3f, (float)i));
    S = plain_filter(S, LS);
    CHECK(S.size() == 40, "premise: 40 surf voxels");
    check_pair("O before the first key", S, {P(-5.f, 0.f, -3.f), P(-4.f, 0.f, -3.f)}, LS, 0, 42);
    check_pair("O after the last key", S, {P(0.f, 0.f, 9.f), P(0.f, 1.f, 9.f)}, LS, 0, 42);
    check_pair("O between keys", S, {P(4.3f, 1.3f, 0.3f), P(-0.3f, 0.3f, 0.3f), P(100.f, 0.3f, 0.3f)}, LS, 0, 43);
    check_pair("several O in one voxel with an S point", S, {P(4.1f, 0.1f, 0.1f), P(12.4f, 0.2f, 0.2f), P(4.2f, 0.2f, 0.2f), P(4.3f, 0.7f, 0.1f)}, LS, 0, 40);
    check_pair("several O in one voxel without an S point", S, {P(4.1f, 1.1f, 0.1f), P(4.2f, 1.2f, 0.2f), P(0.f, -1.f, 0.f), P(4.3f, 0.9f, 0.1f)}, LS, 0, 42);
    check_pair("empty O", S, {}, LS, 0, 40);
    check_pair("empty S", {}, {P(4.1f, 1.1f, 0.1f), P(0.f, 0.f, 0.f), P(4.2f, 1.2f, 0.2f)}, LS, 0, 2);
    check_pair("both empty", {}, {}, LS, 0);
    Cloud big;
    for (int i = 0; i < LT_OCAP + 1; ++i) big.push_back(P(0.8f * (float)(i % 64) + 0.3f, 0.8f * (float)(i / 64) + 0.3f, 2.f));
    check_pair("LT_OCAP + 1 outliers", S, big, LS, 1);
    big.pop_back();
    check_pair("LT_OCAP outliers", S, big, LS, 0);
    check_pair("a cell beyond 2^20", S, {P(1.0e6f, 0.f, 0.f)}, LS, 1);
    check_pair("a cell beyond -2^20", {P(-1.0e6f, 0.f, 0.f)}, {P(-1.0e6f + 1.f, 0.f, 0.f)}, LS, 1);
    check_pair("past the leaf-too-small rule", S, {P(2000.f, 2000.f, 2000.f)}, LS, 1);
    check_pair("a NaN", S, {P(NAN, 0.f, 0.f)}, LS, 1);
  }
  if (fails) { std::printf("vox_merge: %d checks failed\n", fails); return 1; }
  std::printf("vox_merge ok\n");
  return 0;
}
