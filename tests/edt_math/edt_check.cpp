// edt_check.cpp — the rule of csrc/edt_math.h read by a host compiler alone (no HIP runtime), built with AddressSanitizer and UBSan by
// tests/test_edt_math.py.  10^4 random lines of 1 to 70 cells whose values include "none", 0 and values near 2^32 - 2: edt_envelope against the
// O(n^2) definition, with the stack arrays exactly as long as the line (a step outside them is an error the sanitizer reports) and every sep
// numerator asserted non-negative.  Then the lines without a parabola, with one, and with all values equal; the domain rule (unequal edges, the
// 65 537-cell line); pass X's edt_g2; and small grids of the whole twin against every cell and every source.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "edt_math.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return 1; } } while (0)
static int g_case = -1;
static long long g_checks = 0, g_negative = 0;

struct CountingCheck { void operator()(int64_t num) const { ++g_checks; if (num < 0) ++g_negative; } };

// the envelope of f by edt_envelope, stack arrays of exactly n entries
static std::vector<int64_t> envelope(const std::vector<uint32_t>& f) {
  const int32_t n = (int32_t)f.size();
  std::vector<EdtTop> se(n);
  std::vector<int64_t> out(n, -7);
  edt_envelope(n, [&](int32_t u) { return f.at(u); }, [&](int32_t u, int64_t v) { out.at(u) = v; }, EdtHostStack{se.data()}, CountingCheck());
  return out;
}
static std::vector<int64_t> plain(const std::vector<uint32_t>& f) {
  const int n = (int)f.size();
  std::vector<int64_t> out(n, -1);
  for (int u = 0; u < n; ++u)
    for (int i = 0; i < n; ++i) {
      if (f[i] == EDT_FAR) continue;
      const int64_t v = (int64_t)(u - i) * (u - i) + (int64_t)f[i];
      if (out[u] < 0 || v < out[u]) out[u] = v;
    }
  return out;
}

int main() {
  std::mt19937_64 rng(20260);
  // ---- 10^4 random lines
  for (g_case = 0; g_case < 10000; ++g_case) {
    const int n = 1 + (int)(rng() % 70);
    const int kind = (int)(rng() % 5);   // how the finite values are drawn
    const int none_pct = (int)(rng() % 101);
    std::vector<uint32_t> f(n);
    for (int u = 0; u < n; ++u) {
      if ((int)(rng() % 100) < none_pct) { f[u] = EDT_FAR; continue; }
      switch (kind) {
        case 0: f[u] = 0; break;
        case 1: f[u] = (uint32_t)(rng() % 10); break;                                 // close values: long runs of one parabola
        case 2: f[u] = (uint32_t)(rng() % 5000); break;
        case 3: f[u] = 4294967294u - (uint32_t)(rng() % 3000); break;                 // near 2^32 - 2
        default: f[u] = (rng() & 1) ? (uint32_t)(rng() % 4) : 4294967294u - (uint32_t)(rng() % 4); break;   // both ends mixed
      }
    }
    CHECK(envelope(f) == plain(f));
  }
  CHECK(g_negative == 0 && g_checks > 10000);
  // ---- constructed lines
  g_case = -2;
  for (int n = 1; n <= 70; ++n) {
    std::vector<uint32_t> f(n, EDT_FAR);
    const std::vector<int64_t> none = envelope(f);
    for (int u = 0; u < n; ++u) CHECK(none[u] == -1);                                 // no parabola
    for (int at : {0, n / 2, n - 1}) {                                                // one parabola
      std::vector<uint32_t> one(n, EDT_FAR);
      one[at] = 9;
      const std::vector<int64_t> got = envelope(one);
      for (int u = 0; u < n; ++u) CHECK(got[u] == (int64_t)(u - at) * (u - at) + 9);
    }
    for (uint32_t v : {0u, 7u, 4294967294u}) {                                        // all equal: every cell keeps its own value
      const std::vector<int64_t> got = envelope(std::vector<uint32_t>(n, v));
      for (int u = 0; u < n; ++u) CHECK(got[u] == (int64_t)v);
    }
  }
  CHECK(g_negative == 0);
  // ---- the domain
  g_case = -3;
  {
    int32_t dom[3]; double s;
    const int32_t n3[3] = {4, 5, 6}, flat[3] = {4, 5, 1}, linez[3] = {1, 1, 9}, one[3] = {1, 1, 1};
    const double same[3] = {0.2, 0.2, 0.2}, thick[3] = {0.2, 0.2, 3.5}, xy[3] = {0.2, 0.25, 0.2}, z[3] = {0.7, 0.3, 0.5};
    CHECK(!edt_domain(n3, same, 0, dom, &s) && s == 0.2 && dom[2] == 6);
    CHECK(edt_domain(n3, thick, 0, dom, &s) != nullptr);                              // three axes count, one differs
    CHECK(!edt_domain(n3, thick, 1, dom, &s) && s == 0.2 && dom[0] == 4 && dom[1] == 5 && dom[2] == 1);   // collapsed: x and y count
    CHECK(!edt_domain(flat, thick, 0, dom, &s) && s == 0.2);                          // one thick layer
    CHECK(edt_domain(flat, xy, 0, dom, &s) != nullptr && edt_domain(n3, xy, 1, dom, &s) != nullptr);
    CHECK(!edt_domain(linez, z, 0, dom, &s) && s == 0.5);                             // only z counts
    CHECK(!edt_domain(one, z, 0, dom, &s) && s == 0.7);                               // no axis counts: cell[0]
    const int32_t ok_line[3] = {65536, 1, 1}, long_line[3] = {65537, 1, 1}, diag[3] = {65536, 364, 1}, diag_ok[3] = {65536, 363, 1}, zero[3] = {4, 0, 4};
    CHECK(!edt_dims_fault(ok_line, 0) && edt_dims_fault(long_line, 0) && edt_dims_fault(zero, 0));
    CHECK(!edt_dims_fault(diag_ok, 0) && edt_dims_fault(diag, 0));                    // 65535^2 + 362^2 <= 2^32 - 2 < 65535^2 + 363^2
    const int32_t many[3] = {2048, 2048, 512};
    CHECK(edt_dims_fault(many, 0));                                                   // more than 2^31 - 1 cells
    CHECK(edt_dims_fault(n3, -1) && edt_dims_fault(n3, 65536) && !edt_dims_fault(n3, 65535));
  }
  // ---- where a parabola starts: one 32-bit division against the definition's 64-bit one
  g_case = -5;
  for (int t = 0; t < 200000; ++t) {
    const int32_t n = 2 + (int32_t)(rng() % 65535), u = 1 + (int32_t)(rng() % (n - 1)), i = (int32_t)(rng() % u);
    const uint32_t fi = (rng() & 1) ? (uint32_t)(rng() % 100000) : 4294967294u - (uint32_t)(rng() % 100000);
    const int64_t need = (int64_t)fi - ((int64_t)u * u - (int64_t)i * i);   // f(u) >= need keeps the numerator non-negative
    const int64_t fu64 = std::max<int64_t>(need, 0) + (int64_t)(rng() % ((rng() & 1) ? 1000 : 4000000000ull));
    if (fu64 > 4294967294ll) continue;
    const uint32_t fu = (uint32_t)fu64;
    const int64_t num = edt_sep_num(i, fi, u, fu);
    CHECK(num == (int64_t)u * u - (int64_t)i * i + (int64_t)fu - (int64_t)fi && num >= 0);
    const int64_t w = 1 + num / (2 * ((int64_t)u - i));
    CHECK(edt_start(num, i, u, n) == (w < n ? (int32_t)w : n));
  }
  // ---- pass X's rule
  g_case = -4;
  CHECK(edt_g2(5, -1, 9, 9) == EDT_FAR && edt_g2(5, 5, 9, 9) == 0 && edt_g2(5, 2, 9, 9) == 9 && edt_g2(5, -1, 7, 9) == 4 && edt_g2(5, 1, 8, 9) == 9 && edt_g2(5, 1, 6, 9) == 1);
  CHECK(edt_g2(65535, 0, 65536, 65536) == 65535u * 65535u);
  CHECK(edt_cap(10, 0) == 10 && edt_cap(9, 9) == 9 && edt_cap(10, 9) == EDT_FAR && edt_cap(EDT_FAR, 9) == EDT_FAR && edt_cap(0, 1) == 0);
  // ---- the whole twin on small grids, every cell against every source
  for (g_case = 0; g_case < 300; ++g_case) {
    const int32_t n[3] = {1 + (int32_t)(rng() % 7), 1 + (int32_t)(rng() % 7), 1 + (int32_t)(rng() % 7)};
    const int cells = n[0] * n[1] * n[2], pct = (int)(rng() % 101), uio = (int)(rng() & 1), cap = (int)(rng() % 4);
    std::vector<int8_t> cls(cells);
    for (auto& c : cls) c = (int)(rng() % 100) < pct ? 100 : ((rng() & 1) ? 0 : -1);
    std::vector<uint32_t> d2(cells), work(cells);
    std::vector<EdtTop> stack(std::max(n[0], std::max(n[1], n[2])));
    int64_t stats[ALEGO_EDT_STATS];
    edt_distance_host(cls.data(), n, uio, cap, d2.data(), work.data(), stack.data(), stats);
    int64_t far = 0, src = 0, mx = -1;
    for (int i = 0; i < cells; ++i) {
      const int x = i % n[0], y = i / n[0] % n[1], z = i / (n[0] * n[1]);
      int64_t best = -1;
      for (int j = 0; j < cells; ++j) {
        if (!(cls[j] == 100 || (uio && cls[j] == -1))) continue;
        const int dx = x - j % n[0], dy = y - j / n[0] % n[1], dz = z - j / (n[0] * n[1]);
        const int64_t v = dx * dx + dy * dy + dz * dz;
        if (best < 0 || v < best) best = v;
      }
      if (best >= 0 && cap > 0 && best > cap * cap) best = -1;
      CHECK(d2[i] == (best < 0 ? EDT_FAR : (uint32_t)best));
      if (best < 0) ++far; else { if (best == 0) ++src; mx = std::max(mx, best); }
    }
    CHECK(stats[ALEGO_EDT_SOURCES] == src && stats[ALEGO_EDT_FAR_CELLS] == far && stats[ALEGO_EDT_MAX_D2] == mx);
  }
  std::printf("edt ok: %lld sep numerators, none negative\n", g_checks);
  return 0;
}
