// nn_rules_check — csrc/nn_rules.h on the host: the distance, the key, the bounds, the cells, the gates and the ring walk of the nearest-neighbour
// searches, each against its rule written out plainly here.  Built with -ffp-contract=off, ASan and UBSan.  Every check must hold with no exception.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "nn_rules.h"

static long long g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static int rnd(int n) { return (int)(rnd64() % (uint64_t)n); }
static double unit() { return (double)(rnd64() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
static float uni(float a, float b) { return (float)((double)a + ((double)b - (double)a) * unit()); }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float fbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float up(float f) { return nextafterf(f, INFINITY); }
static float dn(float f) { return nextafterf(f, -INFINITY); }
static bool same_f32(float a, float b) { return (isnan(a) && isnan(b)) || bits(a) == bits(b); }
struct P3 { float x, y, z; };

// flann::L2_Simple<float> as a chain of volatile f32 partial sums: nothing is kept wider or fused
static float d2_written_out(P3 a, P3 b) {
  volatile float r = 0.f, df, sq;
  df = a.x - b.x; sq = df * df; r = r + sq;
  df = a.y - b.y; sq = df * df; r = r + sq;
  df = a.z - b.z; sq = df * df; r = r + sq;
  return r;
}

// ---- distance ----
static long long distance() {
  long long n = 0;
  const float sp[] = {0.f, -0.f, fbits(1), -fbits(1), fbits(0x7FFFFF), FLT_MIN, 1.f, -1.f, 0.9f * FLT_MAX, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY, NAN, 1e19f, -1e19f, 1e-19f};
  const int NS = (int)(sizeof(sp) / sizeof(sp[0]));
  std::vector<P3> pts;
  for (int i = 0; i < NS; ++i) for (int j = 0; j < NS; ++j) pts.push_back(P3{sp[i], sp[j], sp[(i + j) % NS]});
  const float scale[] = {1e-22f, 1e-3f, 1.f, 100.f, 4000.f, 1e18f};
  for (int i = 0; i < 600; ++i) { const float s = scale[rnd(6)]; pts.push_back(P3{uni(-s, s), uni(-s, s), uni(-s, s)}); }
  for (size_t i = 0; i < pts.size(); ++i)
    for (int t = 0; t < 40; ++t, ++n) {
      const P3 a = pts[i], b = pts[(i * 7 + (size_t)t * 131 + (size_t)rnd(5)) % pts.size()];
      const float got = nn_d2(a.x, a.y, a.z, b.x, b.y, b.z), want = d2_written_out(a, b);
      CHECK(same_f32(got, want), "nn_d2 (%a %a %a)-(%a %a %a): %a want %a", a.x, a.y, a.z, b.x, b.y, b.z, got, want);
      CHECK(same_f32(nn_d2(b.x, b.y, b.z, a.x, a.y, a.z), want), "nn_d2: the sign of the difference matters");
      volatile float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = xx + yy, g = xy + zz;
      CHECK(same_f32(g, want), "(dx2 + dy2) + dz2 has other bits: %a want %a", (float)g, want);
      CHECK(isnan(got) || bits(got) < 0x80000000u, "nn_d2 is negative or -0");
    }
  return n;
}

// ---- key ----
static long long key() {
  long long n = 0;
  const float D[] = {0.f, fbits(1), dn(1.f), 1.f, up(1.f), FLT_MAX, INFINITY};
  const int I[] = {0, 1, INT_MAX};
  for (float da : D) for (int ia : I) {
    const nn_key_t ka = nn_key(da, (uint32_t)ia);
    CHECK(bits(nn_key_d2(ka)) == bits(da) && nn_key_index(ka) == ia, "key round trip");
    CHECK(ka < NN_NONE, "NN_NONE is not above the key of %a, %d", da, ia);
    for (float db : D) for (int ib : I) {
      ++n;
      const bool lex = da < db || (da == db && ia < ib);
      CHECK((ka < nn_key(db, (uint32_t)ib)) == lex, "key order (%a, %d) (%a, %d)", da, ia, db, ib);
      CHECK(nn_better(da, ia, db, ib) == lex, "nn_better (%a, %d) (%a, %d)", da, ia, db, ib);
    }
  }
  CHECK(nn_key_index(NN_NONE) == -1, "NN_NONE's index is -1");
  // the start states: a key search takes any first candidate, the pair search from (FLT_MAX, -1) none at FLT_MAX, +inf or NaN
  const float edge[] = {FLT_MAX, INFINITY, NAN};
  for (float d : edge) for (int i : I) {
    ++n;
    CHECK(!nn_better(d, i, FLT_MAX, -1), "the pair start state takes %a", d);
    CHECK(nn_key(d, (uint32_t)i) < NN_NONE, "the key start state refuses %a", d);
  }
  CHECK(nn_better(dn(FLT_MAX), 0, FLT_MAX, -1) && nn_better(0.f, INT_MAX, FLT_MAX, -1), "the pair start state refuses a finite candidate below FLT_MAX");
  return n;
}

// ---- bounds ----
static long long g_box_pts = 0, g_face_pts = 0;
static long long bounds() {
  long long n = 0;
  const float scale[] = {1e-21f, 1e-3f, 1.f, 50.f, 4000.f, 1e15f};
  for (int it = 0; it < 4000; ++it) {
    const float s = scale[rnd(6)], c0 = rnd(2) ? 0.f : uni(-40.f * s, 40.f * s);
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      const float u = c0 + uni(-s, s), v = c0 + uni(-s, s);
      lo[a] = fminf(u, v); hi[a] = fmaxf(u, v);
      if (rnd(4) == 0) hi[a] = lo[a];              // degenerate: no extent along this axis
      else if (rnd(8) == 0) hi[a] = up(lo[a]);     // one ulp of extent
    }
    for (int qi = 0; qi < 12; ++qi) {
      float q[3];
      for (int a = 0; a < 3; ++a) {
        const int m = qi < 3 ? 0 : rnd(6);   // 0: inside, 1 / 2: on a face, 3 / 4: outside next to a face, 5: far outside
        q[a] = m == 0 ? uni(lo[a], hi[a]) : m == 1 ? lo[a] : m == 2 ? hi[a] : m == 3 ? dn(lo[a]) : m == 4 ? up(hi[a]) : c0 + uni(-3.f * s, 3.f * s);
        if (m == 0) q[a] = fminf(fmaxf(q[a], lo[a]), hi[a]);
      }
      const float g32[3] = {nn_gap(lo[0], hi[0], q[0]), nn_gap(lo[1], hi[1], q[1]), nn_gap(lo[2], hi[2], q[2])};
      const float lb32 = nn_box_lb(g32[0], g32[1], g32[2]);
      const double lbw = nn_walk_d2(g32[0], g32[1], g32[2]);
      const double lb64 = nn_box_lb_f64(nn_gap_f64(lo[0], hi[0], q[0]), nn_gap_f64(lo[1], hi[1], q[1]), nn_gap_f64(lo[2], hi[2], q[2]));
      for (int a = 0; a < 3; ++a) {   // the gap written out
        const float want = q[a] < lo[a] ? lo[a] - q[a] : q[a] > hi[a] ? q[a] - hi[a] : 0.f;
        CHECK(g32[a] == want, "nn_gap [%a, %a] %a: %a want %a", lo[a], hi[a], q[a], g32[a], want);
      }
      for (int pi = 0; pi < 8 + 27; ++pi, ++n) {
        float p[3];
        for (int a = 0; a < 3; ++a) {
          if (pi < 8) p[a] = (pi >> a) & 1 ? hi[a] : lo[a];   // the corners
          else {
            const int m = (pi - 8) / (a == 0 ? 1 : a == 1 ? 3 : 9) % 3;   // ulp neighbours of the faces, a random point
            p[a] = m == 0 ? up(lo[a]) : m == 1 ? dn(hi[a]) : uni(lo[a], hi[a]);
            p[a] = fminf(fmaxf(p[a], lo[a]), hi[a]);
          }
        }
        ++g_box_pts;
        const float d2 = nn_d2(p[0], p[1], p[2], q[0], q[1], q[2]);
        CHECK(lb32 <= d2, "f32 bound %a above the d2 %a of a point of the box", lb32, d2);
        const double wd = nn_walk_d2(p[0] - q[0], p[1] - q[1], p[2] - q[2]);
        CHECK(lbw <= wd, "f64 walk bound %a above the walk distance %a of a point of the box", lbw, wd);
        CHECK(!nn_beyond(lb64, d2) && !nn_beyond(lb64, up(d2)), "the loop bound %a declares a point at d2 %a beyond", lb64, d2);
      }
    }
  }
  // the half-space bound of the loop grid: no point of a cell beyond the face is declared beyond its own d2
  for (int it = 0; it < 3000; ++it) {
    const int k = rnd(14) - 9, g = 1 + rnd(40);
    const double h = ldexp(1.0, k), inv_h = ldexp(1.0, -k);
    const float mnf = rnd(3) ? uni(-300.f, 300.f) : 0.f;
    const double mn = mnf, slack = nn_face_slack(mn, (double)g * h, h);
    const float q = (float)(mn + (unit() * (g + 4) - 2.0) * h);
    const int c = nn_lc_axis(q, mn, inv_h, g);
    for (int t = 0; t < 30; ++t) {
      float x = (float)(mn + unit() * g * h);
      if (rnd(4) == 0) x = (float)(mn + rnd(g + 1) * h);   // on a face
      if (rnd(8) == 0) x = dn(x);
      if (x < mnf) x = mnf;
      const int cx = nn_lc_axis(x, mn, inv_h, g);
      const float d2 = nn_d2(x, 0.f, 0.f, q, 0.f, 0.f);
      for (int r = 0; r < g; ++r) {
        if (cx >= c + r + 1) { ++g_face_pts; CHECK(!nn_beyond(nn_face_lb((mn + (double)(c + r + 1) * h) - (double)q, slack), d2), "upper half-space bound: a point beyond it at d2 %a", d2); }
        if (cx <= c - r - 1) { ++g_face_pts; CHECK(!nn_beyond(nn_face_lb((double)q - (mn + (double)(c - r) * h), slack), d2), "lower half-space bound: a point beyond it at d2 %a", d2); }
      }
    }
  }
  return n;
}

// ---- cells ----
static long long g_lm_pairs = 0, g_lo_near = 0, g_lc = 0;
static long long cells() {
  long long n = 0;
  // LaserMapping: pairs closer than the limit are at most one cell apart along every axis
  const double kmds[] = {1.0, 0.7, 1.1, 2.0 / 3.0, 4.0};
  for (double kmd : kmds) {
    const float cell = nn_lm_cell(kmd), inv = 1.0f / cell;
    const uint32_t lim = nn_lm_limit_bits(kmd);
    int cell_exp;
    CHECK((double)cell * cell >= kmd && (cell == 1.0f || (double)(cell / 2) * (cell / 2) < kmd) && frexpf(cell, &cell_exp) == 0.5f, "cell size %a for %a", cell, kmd);
    const float flim = fbits(lim);
    const float gate[] = {dn(dn(flim)), dn(flim), flim, up(flim), 0.f, fbits(1), (float)kmd, INFINITY};
    for (float d : gate) { ++n; CHECK(nn_lm_within(d, lim) == ((double)d < kmd), "limit bits: d2 %a against %a", d, kmd); }
    CHECK(nn_lm_row_ok(3, dn(flim), kmd) && !nn_lm_row_ok(3, flim, kmd) && !nn_lm_row_ok(-1, 0.f, kmd) && !nn_lm_row_ok(nn_key_index(NN_NONE), nn_key_d2(NN_NONE), kmd), "accepted-row rule");
    const float r = (float)sqrt(kmd);
    const float base[] = {0.f, 1.f, 2.f, 4.f, 8.f, 64.f, 1024.f, 4000.f, 4096.f, -1.f, -2.f, -64.f, -4000.f, -4096.f, 0.5f, 0.25f, 3.f * cell, -5.f * cell, 1000.f * cell};
    for (float b : base)
      for (int t = 0; t < 800; ++t) {
        float q[3], p[3];
        for (int a = 0; a < 3; ++a) {
          const int m = rnd(5);   // the query on either side of a binade / cell boundary, or anywhere near it
          q[a] = m == 0 ? b : m == 1 ? dn(b) : m == 2 ? up(b) : m == 3 ? b + uni(-cell, cell) : (float)rnd(9) * cell - 4.f * cell + b;
          const int w = rnd(8);
          const float mag = w == 0 ? cell : w == 1 ? dn(cell) : w == 2 ? r : w == 3 ? dn(r) : w == 4 ? up(r) : w == 5 ? 0.f : uni(0.f, r);
          p[a] = q[a] + (rnd(2) ? mag : -mag);
          if (rnd(6) == 0) p[a] = rnd(2) ? up(p[a]) : dn(p[a]);
        }
        if (rnd(4)) { const int a = rnd(3); for (int o = 0; o < 3; ++o) if (o != a) p[o] = q[o] + uni(-0.01f, 0.01f); }   // (mostly one axis: d2 stays below the limit)
        ++n;
        if (!nn_lm_within(nn_d2(q[0], q[1], q[2], p[0], p[1], p[2]), lim)) continue;
        ++g_lm_pairs;
        for (int a = 0; a < 3; ++a) {
          const long long dc = (long long)nn_lm_coord(q[a], inv) - nn_lm_coord(p[a], inv);
          CHECK(dc >= -1 && dc <= 1, "LM cells: %a and %a are %lld cells of %a apart at a d2 below %a", q[a], p[a], dc, cell, kmd);
        }
      }
  }
  CHECK(nn_lm_limit_bits(0.0) == 0u && nn_lm_limit_bits(-1.0) == 0u && !nn_lm_within(0.f, 0u), "a limit of 0 lets nothing pass");
  CHECK(nn_lm_coord(3e38f, 1.f) == 1073741824 && nn_lm_coord(-3e38f, 1.f) == -1073741824 && nn_lm_coord(-0.5f, 1.f) == -1 && nn_lm_coord(7.9f, 0.25f) == 1, "nn_lm_coord");
  CHECK(nn_lm_index(-3, 5, 1, 4, 5, 6) == 0 + 4 * (4 + 5 * 1) && nn_lm_index(2, 1, 9, 4, 5, 6) == 2 + 4 * (1 + 5 * 5), "nn_lm_index clamps");
  // LaserOdometry: every target below the settle threshold lies in the 3 x 3 cells the query looks at (lo_assoc's cell addressing written out)
  const float cszs[] = {1.f, 2.f, 8.f};
  for (float csz : cszs)
    for (int it = 0; it < 300; ++it) {
      const float inv = 1.0f / csz, settle = nn_lo_settle(csz);
      { volatile float s = 0.999f, t = s * csz, u = t * csz; CHECK(settle == u, "settle threshold"); }
      const bool thin = rnd(2);
      const float ex = (thin ? 2000.f : 60.f) * csz * (float)unit(), ey = (thin ? 1.f : 60.f) * csz * (float)unit();
      const float ox = uni(-3000.f, 3000.f), oy = uni(-3000.f, 3000.f);
      std::vector<P3> tg;
      for (int i = 0; i < 60; ++i) {
        P3 t{ox + ex * (float)unit(), oy + ey * (float)unit(), uni(-2.f, 2.f)};
        if (rnd(3) == 0) { t.x = ox + floorf(ex * (float)unit() / csz) * csz; if (rnd(2)) t.x = dn(t.x); }   // next to a cell boundary
        if (rnd(3) == 0) { t.y = oy + floorf(ey * (float)unit() / csz) * csz; if (rnd(2)) t.y = up(t.y); }
        tg.push_back(t);
      }
      float mn[2] = {FLT_MAX, FLT_MAX}, mx[2] = {-FLT_MAX, -FLT_MAX};
      for (const P3& t : tg) { mn[0] = fminf(mn[0], t.x); mn[1] = fminf(mn[1], t.y); mx[0] = fmaxf(mx[0], t.x); mx[1] = fmaxf(mx[1], t.y); }
      const int gx = (int)floorf((mx[0] - mn[0]) / csz) + 2, gy = (int)floorf((mx[1] - mn[1]) / csz) + 2;   // lo_grid_build
      if ((long long)gx * gy > 4096) continue;
      for (int qi = 0; qi < 200; ++qi, ++n) {
        const P3& near = tg[rnd((int)tg.size())];
        const int w = rnd(4);
        const float reach = w == 0 ? 0.9995f * csz : w == 1 ? 0.99949f * csz : w == 2 ? csz : csz * (float)unit();
        const int dir = rnd(4);
        P3 q{near.x + (dir == 0 ? reach : dir == 1 ? -reach : uni(-reach, reach)), near.y + (dir == 2 ? reach : dir == 3 ? -reach : uni(-0.02f, 0.02f) * csz), near.z + uni(-0.01f, 0.01f)};
        if (rnd(10) == 0) q.x = rnd(2) ? mn[0] - csz * (float)unit() : mn[0] + ((float)(gx - 1) + (float)unit()) * csz;   // up to one cell outside the grid
        if (rnd(10) == 0) q.y = rnd(2) ? mn[1] - csz * (float)unit() : mn[1] + ((float)(gy - 1) + (float)unit()) * csz;
        const int cx = nn_lo_cell(q.x, mn[0], inv), cy = nn_lo_cell(q.y, mn[1], inv);
        const int x0 = std::max(cx - 1, 0), x1 = std::min(cx + 1, gx - 1);
        for (const P3& t : tg) {
          const int ux = nn_lo_cell(t.x, mn[0], inv), uy = nn_lo_cell(t.y, mn[1], inv);
          CHECK(ux >= 0 && ux < gx && uy >= 0 && uy < gy, "the build's clamp moves a target");
          if (!(nn_d2(t.x, t.y, t.z, q.x, q.y, q.z) < settle)) continue;
          ++g_lo_near;
          const int r = uy - cy + 1;   // the row of the 3 x 3 block that has to hold it
          const bool in = r >= 0 && r < 3 && uy >= 0 && uy < gy && x0 <= x1 && cx >= -1 && cx <= gx && ux >= x0 && ux <= x1;
          CHECK(in, "LO cells (csz %g): target cell (%d, %d) outside the 3 x 3 cells of query cell (%d, %d), grid %d x %d", csz, ux, uy, cx, cy, gx, gy);
        }
      }
    }
  // the loop grid: the cell of a point is the f64 formula evaluated in long double
  for (int it = 0; it < 200000; ++it, ++g_lc) {
    const int k = rnd(17) - 10, g = 1 + rnd(300);
    const double mn = rnd(4) ? (double)uni(-500.f, 500.f) : (double)uni(-1e-3f, 1e-3f);
    const long double h = ldexpl(1.0L, k);
    float x = (float)((long double)mn + ((long double)unit() * (g + 2) - 1.0L) * h);
    if (rnd(4) == 0) x = (float)((long double)mn + (long double)rnd(g + 1) * h);
    if (rnd(8) == 0) x = rnd(2) ? up(x) : dn(x);
    long double v = floorl(((long double)x - (long double)mn) * ldexpl(1.0L, -k));
    if (v < 0) v = 0;
    if (v > g - 1) v = g - 1;
    CHECK(nn_lc_axis(x, mn, ldexp(1.0, -k), g) == (int)v, "loop cell of %a from %a, h 2^%d: %d want %d", x, mn, k, nn_lc_axis(x, mn, ldexp(1.0, -k), g), (int)v);
  }
  CHECK(nn_lc_axis(NAN, 0.0, 1.0, 5) == 0 && nn_lc_axis(INFINITY, 0.0, 1.0, 5) == 4 && nn_lc_axis(-INFINITY, 0.0, 1.0, 5) == 0, "loop cell of a non-finite coordinate");
  CHECK(nn_lc_index(1, 2, 3, 4, 5) == (3 * 5 + 2) * 4 + 1, "nn_lc_index");
  // its choice of k: the cell count at 2^k is within the target at every size from "one cell" down to k, and not at 2^(k-1)
  for (int it = 0; it < 20000; ++it, ++n) {
    double e[3], emax = 0.0;
    const double s = ldexp(1.0, rnd(30) - 15);
    for (int a = 0; a < 3; ++a) { e[a] = rnd(5) ? s * unit() : 0.0; emax = fmax(emax, e[a]); }
    const double target = (double)(1 + rnd(rnd(2) ? 8 : 5000));
    const int k = nn_lc_cell_exp(e, emax, target);
    auto count = [&](int kk) { double c = 1.0; for (int a = 0; a < 3; ++a) c *= floor(e[a] / ldexp(1.0, kk)) + 1.0; return c; };
    const int k0 = emax > 0.0 ? ilogb(emax) + 1 : 0;
    CHECK(k <= k0 && count(k0) == 1.0, "2^k0 is one cell");
    for (int kk = k; kk < k0; ++kk) CHECK(count(kk) <= target, "k %d: %g cells at 2^%d, target %g", k, count(kk), kk, target);
    CHECK(count(k - 1) > target || k - 1 < -120, "k %d is not the smallest: %g cells at 2^%d, target %g", k, count(k - 1), k - 1, target);
  }
  return n;
}

// ---- the ring walk against the reference's two loops (laserOdometry.cpp:344-373 surf, :433-475 corner; ring_window for their 2) ----
static long long g_walk_rows = 0, g_walk_ties = 0;
static long long walk() {
  long long n = 0;
  const int NS = 6;
  const int Ws[] = {0, 1, 2, 100};
  for (int it = 0; it < 6000; ++it) {
    const int np = 1 + rnd(40);
    std::vector<P3> pt(np);
    std::vector<int> ring(np);
    for (int i = 0; i < np; ++i) ring[i] = rnd(NS);
    std::sort(ring.begin(), ring.end());
    for (int i = 0; i < np; ++i) pt[i] = P3{0.25f * (float)rnd(6), 0.25f * (float)rnd(3), 0.5f * (float)rnd(2)};   // few distinct points: many ties
    int roff[NS + 1];
    for (int r = 0; r <= NS; ++r) roff[r] = (int)(std::lower_bound(ring.begin(), ring.end(), r) - ring.begin());
    const P3 sel{uni(-0.2f, 1.5f), uni(-0.2f, 0.7f), uni(-0.2f, 0.7f)};
    const int cm = rnd(4), closest = cm == 0 ? 0 : cm == 1 ? np - 1 : rnd(np);
    const double nfd = rnd(3) ? 25.0 : 0.3;
    for (int kind = 0; kind < 2; ++kind)
      for (int W : Ws) {
        ++n;
        // the reference
        int min_idx2 = -1, min_idx3 = -1;
        {
          double point_dist, min_dist2 = nfd, min_dist3 = nfd;
          const int closest_scan = ring[closest];
          auto dist = [&](int k) { return pow(pt[k].x - sel.x, 2) + pow(pt[k].y - sel.y, 2) + pow(pt[k].z - sel.z, 2); };
          for (int k = closest + 1; k < np; ++k) {
            if (ring[k] > closest_scan + W) break;
            point_dist = dist(k);
            if (kind == 0) {
              if (ring[k] == closest_scan) { if (point_dist < min_dist2) { min_dist2 = point_dist; min_idx2 = k; } }
              else { if (point_dist < min_dist3) { min_dist3 = point_dist; min_idx3 = k; } }
            } else if (ring[k] > closest_scan) { if (point_dist < min_dist2) { min_dist2 = point_dist; min_idx2 = k; } }
          }
          for (int k = closest - 1; k >= 0; --k) {
            if (ring[k] < closest_scan - W) break;
            point_dist = dist(k);
            if (kind == 0) {
              if (ring[k] == closest_scan) { if (point_dist < min_dist2) { min_dist2 = point_dist; min_idx2 = k; } }
              else { if (point_dist < min_dist3) { min_dist3 = point_dist; min_idx3 = k; } }
            } else if (ring[k] < closest_scan) { if (point_dist < min_dist2) { min_dist2 = point_dist; min_idx2 = k; } }
          }
        }
        // the header's rules: an arg-min over (distance, rank) per class, candidates in any order
        const int cr = ring[closest];
        const int rlo = nn_walk_ring(cr, -W, NS), rhi = nn_walk_ring(cr, W, NS), own = nn_walk_ring(cr, 0, NS);
        const int lo = roff[rlo], hi = roff[rhi + 1], same_lo = roff[own], same_hi = roff[own + 1];
        std::vector<int> order;
        for (int k = lo; k < hi; ++k) if (k != closest) order.push_back(k);
        for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[(size_t)rnd((int)i)]);
        double d2b = nfd, d3b = nfd;
        int r2 = INT_MAX, r3 = INT_MAX, i2 = -1, i3 = -1;
        for (int k : order) {
          const double pd = nn_walk_d2(pt[k].x - sel.x, pt[k].y - sel.y, pt[k].z - sel.z);
          if (!(pd < nfd)) continue;
          const int rank = nn_walk_rank(k, closest, hi);
          const bool same = k >= same_lo && k < same_hi;
          if (pd == d2b || pd == d3b) ++g_walk_ties;
          if (nn_walk_second(kind, same) && nn_walk_better(pd, rank, d2b, r2)) { d2b = pd; r2 = rank; i2 = k; }
          if (nn_walk_third(kind, same) && nn_walk_better(pd, rank, d3b, r3)) { d3b = pd; r3 = rank; i3 = k; }
        }
        CHECK(i2 == min_idx2 && i3 == min_idx3, "walk kind %d W %d closest %d of %d: (%d, %d) want (%d, %d)", kind, W, closest, np, i2, i3, min_idx2, min_idx3);
        CHECK(nn_lo_row_ok(kind, i2, i3) == (kind == 0 ? (min_idx2 >= 0 && min_idx3 >= 0) : (min_idx2 >= 0)), "row-accepted rule");
        if (nn_lo_row_ok(kind, i2, i3)) ++g_walk_rows;
      }
  }
  // the visiting rank is a numbering of the walk: closest + 1, + 2, ... then closest - 1, - 2, ...
  for (int hi = 1; hi < 12; ++hi) for (int c = 0; c < hi; ++c) {
    int want = 0;
    for (int k = c + 1; k < hi; ++k, ++want) CHECK(nn_walk_rank(k, c, hi) == want, "rank going up");
    for (int k = c - 1; k >= 0; --k, ++want) CHECK(nn_walk_rank(k, c, hi) == want, "rank going down");
  }
  return n;
}

// ---- gates ----
static long long gates() {
  long long n = 0;
  const double nfds[] = {25.0, 0.1, 1e-3, 1.0};
  for (double nfd : nfds) {
    const float f = (float)nfd;
    const float d[] = {dn(f), f, up(f), 0.f, INFINITY, NAN};
    for (float v : d) { ++n; CHECK(nn_lo_found(v, nfd) == ((double)v < nfd), "nn_lo_found"); }
  }
  const double radii[] = {7.0, 0.1, 50.0, 1e-3, 3.3};
  for (double r : radii) {
    volatile double rr = r * r;
    const float r2 = (float)rr;
    CHECK(nn_r2(r) == r2, "nn_r2");
    const float d[] = {dn(r2), r2, up(r2), 0.f, INFINITY, NAN};
    for (float v : d) { ++n; CHECK(nn_in_radius(v, r2) == (v < r2), "nn_in_radius"); }
  }
  CHECK(!nn_in_radius(NAN, 1.f) && !nn_lo_found(NAN, 1.0), "NaN passes no gate");
  return n;
}

int main() {
  const long long nd = distance(); printf("distance: %lld pairs\n", nd);
  const long long nk = key(); printf("key: %lld ordered pairs and start states\n", nk);
  const long long nb = bounds(); printf("bounds: %lld (box, query, point) cases, %lld points of boxes, %lld points beyond a face\n", nb, g_box_pts, g_face_pts);
  const long long nc = cells(); printf("cells: %lld cases; LM %lld pairs below the limit; LO %lld targets below the settle threshold; loop %lld points\n", nc, g_lm_pairs, g_lo_near, g_lc);
  const long long nw = walk(); printf("walk: %lld walks, %lld accepted rows, %lld ties\n", nw, g_walk_rows, g_walk_ties);
  const long long ng = gates(); printf("gates: %lld\n", ng);
  CHECK(g_lm_pairs > 20000 && g_lo_near > 20000 && g_face_pts > 20000 && g_walk_rows > 5000 && g_walk_ties > 5000, "a check ran on too few cases");
  if (g_fail) { printf("nn_rules: %lld FAILED\n", g_fail); return 1; }
  printf("nn_rules ok\n");
  return 0;
}
