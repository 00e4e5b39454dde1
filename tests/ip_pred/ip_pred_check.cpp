// ip_pred_check — csrc/ip_pred.h on the host: whenever an f32 screen decides, its answer is the full decision (fp64 margins with their fall-through to the
// reference expression), a decided site lies outside the fp64 margin band, and every special or disabled input is left undecided.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ip_pred.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static double rnd01() { return (double)(rnd64() >> 11) * (1.0 / 9007199254740992.0); }
static float ulps(float v, int n) {   // v moved by n units in the last place (v > 0, the result stays positive and finite in every use here)
  int32_t b; memcpy(&b, &v, 4); b += n; float r; memcpy(&r, &b, 4); return r;
}

struct EdgeSet { double ax, ay, theta; };
struct EdgeStat { long long n = 0, und = 0; };

// one site, as the kernels evaluate it: the screen on the f32 ranges, the full decision on their fp64 conversions
static void edge_site(float d1, float d2, double sa, double ca, double theta, double tan_theta, float kh, float kl, float band, EdgeStat* st) {
  const IpScreenBits s = ip_edge_screen(d1, d2, kh, kl, band);
  ++st->n;
  if (s.und) { ++st->und; CHECK(!s.yes, "undecided site says yes"); return; }
  const double y = (double)d2 * sa, x = (double)d1 - (double)d2 * ca;
  const bool full = edge_angle_gt(y, x, theta, tan_theta);
  CHECK(s.yes == full, "edge: d1 %.9g d2 %.9g theta %g sin a %g: screen %d, full %d", d1, d2, theta, sa, (int)s.yes, (int)full);
  CHECK(edge_angle_margin(y, x, tan_theta) >= 0, "edge: d1 %.9g d2 %.9g theta %g sin a %g: decided inside the fp64 band", d1, d2, theta, sa);
}

static void edge_specials(float kh, float kl, float band, bool disabled) {
  const float nanf_ = NAN, inff = INFINITY, den = 1e-40f, dmin = 1.4e-45f;
  const float sp[] = {0.0f, dmin, den, 1.1e-38f, inff, nanf_};
  const float ok[] = {0.3f, 1.0f, 5.0f, 200.0f};
  for (float a : sp) {
    for (float b : sp) CHECK(ip_edge_screen(a, b, kh, kl, band).und, "edge special (%g, %g) decided", a, b);
    for (float b : ok) {
      // (the predicate's premise is d1 >= d2: a special value that is the smaller one sits in d2, the larger in d1)
      const bool a_small = !(a > b);
      CHECK(ip_edge_screen(a_small ? b : a, a_small ? a : b, kh, kl, band).und, "edge special (%g with %g) decided", a, b);
      if (a != a) CHECK(ip_edge_screen(a, b, kh, kl, band).und, "edge special (NaN, %g) decided", b);
    }
  }
  if (disabled) {
    for (float a : ok) for (float b : ok) if (a >= b) CHECK(ip_edge_screen(a, b, kh, kl, band).und, "disabled edge screen decided (%g, %g)", a, b);
  }
}

static void run_edges() {
  const double deg = M_PI / 180.0;
  const EdgeSet sets[4] = {
    {0.2 * deg, 2.0 * deg, 1.047},                  // the defaults: 16 x 1800
    {0.09 * deg, 2.0 * deg, 1.047},                 // 16 x 4000
    {360.0 / 2048 * deg, 26.8 / 63 * deg, 1.047},   // 64 x 2048
    {0.2 * deg, 2.0 * deg, 0.05},                   // a small tan(theta)
  };
  for (const EdgeSet& S : sets) {
    const double tan_theta = tan(S.theta);
    const IpScreenConsts c = ip_screen_consts(sin(S.ax), cos(S.ax), sin(S.ay), cos(S.ay), tan_theta, tan(-10 * deg), tan(10 * deg), 1);
    CHECK(c.eband > 0.0f && c.eband < 1e-6f, "edge screen not enabled for theta %g", S.theta);
    EdgeStat near, uni, eq;
    for (int k = 0; k < 2; ++k) {
      const double a = k ? S.ay : S.ax, sa = sin(a), ca = cos(a);
      const float kh = k ? c.kyh : c.kxh, kl = k ? c.kyl : c.kxl;
      const double K = (sa + ca * tan_theta) / tan_theta;
      // d2 over 10000 f32 values from 0.3 m to 200 m, d1 at every f32 within 64 ulps of d2 K; and d1 = d2
      const int ND = 10000;
      for (int i = 0; i < ND; ++i) {
        const float d2 = (float)(0.3 * pow(200.0 / 0.3, (i + rnd01()) / ND));
        const float mid = (float)((double)d2 * K);
        for (int u = -64; u <= 64; ++u) { const float d1 = ulps(mid, u); if (d1 >= d2) edge_site(d1, d2, sa, ca, S.theta, tan_theta, kh, kl, c.eband, &near); }
        edge_site(d2, d2, sa, ca, S.theta, tan_theta, kh, kl, c.eband, &eq);
      }
      // 10^7 random pairs over the four sets and two angles: ratios uniform in [1, 1.05]
      for (int i = 0; i < 1250000; ++i) {
        const float d2 = (float)(0.3 * pow(200.0 / 0.3, rnd01()));
        float d1 = (float)((double)d2 * (1.0 + 0.05 * rnd01()));
        if (d1 < d2) d1 = d2;
        edge_site(d1, d2, sa, ca, S.theta, tan_theta, kh, kl, c.eband, &uni);
      }
      edge_specials(kh, kl, c.eband, false);
    }
    const double fu = (double)uni.und / (double)uni.n;
    printf("edges ax %.4f ay %.4f theta %.3f band %.3g: within 64 ulps %lld sites, %.4f %% undecided; uniform ratios %lld sites, %.3g undecided; d1 = d2: %lld undecided of %lld\n",
           S.ax / deg, S.ay / deg, S.theta, (double)c.eband, near.n, 100.0 * near.und / near.n, uni.n, fu, eq.und, eq.n);
    CHECK(fu < 1e-5, "uniform ratios: %g of the sites undecided", fu);
    CHECK(near.und < near.n / 20, "the screen decides almost nothing next to the threshold");
  }
  // theta outside (0, 1.5): alego_create hands tan_theta = NaN; seg_alpha outside (0, pi/2); the switch
  const double sa = sin(0.2 * deg), ca = cos(0.2 * deg), say = sin(2 * deg), cay = cos(2 * deg);
  const double bad_tan[] = {NAN, 0.0, -0.5, INFINITY, 1e4};
  for (double t : bad_tan) {
    const IpScreenConsts c = ip_screen_consts(sa, ca, say, cay, t, tan(-10 * deg), tan(10 * deg), 1);
    edge_specials(c.kxh, c.kxl, c.eband, true); edge_specials(c.kyh, c.kyl, c.eband, true);
  }
  {
    const IpScreenConsts c = ip_screen_consts(sin(-0.1), cos(-0.1), say, cay, tan(1.047), tan(-10 * deg), tan(10 * deg), 1);
    edge_specials(c.kxh, c.kxl, c.eband, true); edge_specials(c.kyh, c.kyl, c.eband, true);
    const IpScreenConsts z = ip_screen_consts(sa, ca, say, cay, tan(1.047), tan(-10 * deg), tan(10 * deg), 0);
    edge_specials(z.kxh, z.kxl, z.eband, true); edge_specials(z.kyh, z.kyl, z.eband, true);
  }
}

struct GroundStat { long long n = 0, und = 0; };
static void ground_site(const IpScreenConsts& c, double tl, double th, double mount, double thres, float fx, float fy, float fz, GroundStat* st) {
  const IpScreenBits s = ip_ground_screen(c.g_lo, c.g_hi, c.g_max, fx, fy, fz);
  ++st->n;
  if (s.und) { ++st->und; CHECK(!s.yes, "undecided pair says yes"); return; }
  const bool full = ip_ground_decide(tl, th, mount, thres, fx, fy, fz);
  CHECK(s.yes == full, "ground: (%.9g, %.9g, %.9g) mount %g thres %g: screen %d, full %d", fx, fy, fz, mount, thres, (int)s.yes, (int)full);
  CHECK(ip_ground_margins(tl, th, fx, fy, fz) >= 0, "ground: (%.9g, %.9g, %.9g) mount %g thres %g: decided inside the fp64 band", fx, fy, fz, mount, thres);
}
static void ground_specials(const IpScreenConsts& c, bool disabled) {
  const float v[] = {0.0f, -0.0f, 1.4e-45f, -1e-40f, 1e-39f, 2e19f, -1e30f, 3e38f, INFINITY, -INFINITY, NAN};
  const int nsmall = 5, nv = (int)(sizeof(v) / sizeof(v[0]));
  // zero / denormal vectors in every combination; a huge or non-finite component next to ordinary ones
  for (int i = 0; i < nsmall; ++i) for (int j = 0; j < nsmall; ++j) for (int k = 0; k < nsmall; ++k)
    CHECK(ip_ground_screen(c.g_lo, c.g_hi, c.g_max, v[i], v[j], v[k]).und, "ground special (%g, %g, %g) decided", v[i], v[j], v[k]);
  for (int i = nsmall; i < nv; ++i) {
    CHECK(ip_ground_screen(c.g_lo, c.g_hi, c.g_max, v[i], 0.3f, 0.01f).und, "ground special x = %g decided", v[i]);
    CHECK(ip_ground_screen(c.g_lo, c.g_hi, c.g_max, 0.3f, v[i], 0.01f).und, "ground special y = %g decided", v[i]);
    CHECK(ip_ground_screen(c.g_lo, c.g_hi, c.g_max, 0.3f, -0.2f, v[i]).und, "ground special z = %g decided", v[i]);
    CHECK(ip_ground_screen(c.g_lo, c.g_hi, c.g_max, v[i], v[i], v[i]).und, "ground special all = %g decided", v[i]);
  }
  if (disabled) {
    const float o[] = {-1.0f, -0.05f, 0.0f, 0.02f, 0.7f};
    for (float x : o) for (float y : o) for (float z : o) CHECK(ip_ground_screen(c.g_lo, c.g_hi, c.g_max, x, y, z).und, "disabled ground screen decided (%g, %g, %g)", x, y, z);
  }
}
static void run_ground() {
  const double deg = M_PI / 180.0;
  const double sets[4][2] = {{0.0, 10.0}, {5.0, 10.0}, {-15.0, 3.0}, {20.0, 20.0}};   // (sensor_mount_ang, ground_angle_thres); the last has a bound at 0 degrees
  for (const auto& S : sets) {
    const double mount = S[0], thres = S[1], tl = tan((mount - thres) * deg), th = tan((mount + thres) * deg);
    const IpScreenConsts c = ip_screen_consts(sin(0.2 * deg), cos(0.2 * deg), sin(2 * deg), cos(2 * deg), tan(1.047), tl, th, 1);
    CHECK(c.g_max == c.g_max, "ground screen not enabled for mount %g thres %g", mount, thres);
    GroundStat nearb, wide;
    for (int b = 0; b < 2; ++b) {
      const double tb = b ? th : tl;
      for (int i = 0; i < 200000; ++i) {   // slopes within 1e-5 (relative) of the bound, h from 1e-3 m to 1e2 m; then the f32 neighbours of the bound itself
        const double h = 1e-3 * pow(1e5, rnd01()), phi = 2 * M_PI * rnd01();
        const float fx = (float)(h * cos(phi)), fy = (float)(h * sin(phi));
        const double hh = hypot((double)fx, (double)fy);
        const float fz = (float)(tb * hh * (1.0 + 1e-5 * (2 * rnd01() - 1)));
        ground_site(c, tl, th, mount, thres, fx, fy, fz, &nearb);
        if (tb != 0.0 && (i & 7) == 0) {
          const float fb = (float)(tb * hh);
          for (int u = -3; u <= 3; ++u) { float z; int32_t q; memcpy(&q, &fb, 4); q += u; memcpy(&z, &q, 4); ground_site(c, tl, th, mount, thres, fx, fy, z, &nearb); }
        } else if ((i & 7) == 0) {
          const float zs[] = {0.0f, -0.0f, 1e-40f, -1e-40f, 1e-12f, -1e-12f};
          for (float z : zs) ground_site(c, tl, th, mount, thres, fx, fy, z, &nearb);
        }
      }
    }
    for (int i = 0; i < 500000; ++i) {   // slopes anywhere
      const double h = 1e-3 * pow(1e5, rnd01()), phi = 2 * M_PI * rnd01(), el = (rnd01() - 0.5) * M_PI;
      ground_site(c, tl, th, mount, thres, (float)(h * cos(phi)), (float)(h * sin(phi)), (float)(h * tan(el)), &wide);
    }
    printf("ground mount %g thres %g: within 1e-5 of a bound %lld pairs, %.3f %% undecided; anywhere %lld pairs, %.3g undecided\n",
           mount, thres, nearb.n, 100.0 * nearb.und / nearb.n, wide.n, (double)wide.und / wide.n);
    // (sanity, not a property of the decision: around a bound tan b the tolerance leaves slopes within ~ 4e-6 (tan^2 b + g_max) / (2 tan^2 b) undecided, a
    //  few 1e-5 of all elevations — but |slope| < sqrt(4e-6 g_max), 1e-3 of them, around a bound at 0 degrees, where the signed square is flat)
    if (fabs(tl) > 0.05 && fabs(th) > 0.05) CHECK(wide.und < wide.n / 1000, "the ground screen leaves %lld of %lld ordinary pairs undecided", wide.und, wide.n);
    ground_specials(c, false);
  }
  {
    const IpScreenConsts n = ip_screen_consts(sin(0.2 * deg), cos(0.2 * deg), sin(2 * deg), cos(2 * deg), tan(1.047), NAN, NAN, 1);
    ground_specials(n, true);
    const IpScreenConsts z = ip_screen_consts(sin(0.2 * deg), cos(0.2 * deg), sin(2 * deg), cos(2 * deg), tan(1.047), tan(-10 * deg), tan(10 * deg), 0);
    ground_specials(z, true);
  }
}

int main() {
  run_edges();
  run_ground();
  if (g_fail) { printf("ip_pred: %d checks failed\n", g_fail); return 1; }
  printf("ip_pred ok\n");
  return 0;
}
