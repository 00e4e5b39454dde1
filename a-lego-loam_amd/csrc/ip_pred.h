// ip_pred.h — the two per-cell decisions of ImageProjection's phase B: the ground test of two vertically adjacent cells and the
// segmentation's edge predicate of two neighbouring ranges.  Each exists twice: the fp64 margin form with its fall-through to the reference's
// own atan2 expression (the decision every path agrees on), and an f32 screen that either delivers that same decision or says "undecided".
// Readable by a host compiler without the HIP runtime: tests/ip_pred/ip_pred_check.cpp runs the screens against the full decisions on the CPU.
#ifndef ALEGO_IP_PRED_H_
#define ALEGO_IP_PRED_H_

#ifdef __HIPCC__
#define IP_PRED_FN __device__ __forceinline__
#define IP_PRED_REF __device__ __attribute__((noinline)) inline
#define IP_PRED_HOST __host__ inline
#else
#include <math.h>
#define IP_PRED_FN inline
#define IP_PRED_REF inline
#define IP_PRED_HOST inline
#endif

// ground test of two vertically adjacent cells (imageProjection.cpp:111-131): |deg(atan2(dz, hypot(dx, dy))) - mount| < thres
// <=> tan(lo) h < dz < tan(hi) h; decided by the two signed margins unless one of them is within 1e-9 (relative) of zero, where
// the reference expression decides.  fx, fy, fz = the f32 differences upper - lower.
// (the reference expressions themselves are real calls, not inlined: they are taken by a vanishing fraction of the cells, and inlined into
//  the unrolled per-row code of ip_fused / ip_front their fp64 atan2 / hypot bodies were 90 % of those kernels' instructions and the
//  source of their register spills)
IP_PRED_REF bool ip_is_ground_ref(double dx, double dy, double dz, double mount, double thres) {
  const double angle = (atan2(dz, hypot(dx, dy)) * 180.0) / M_PI;
  return fabs(angle - mount) < thres;
}
IP_PRED_REF bool edge_angle_ref(double y, double x, double theta) { return atan2(y, x) > theta; }
// (round 5: the two margins are taken in "signed square" space — f(x) = sign(x) x^2 is strictly increasing, so f(dz) - f(tan h) has the sign of dz - tan h —
//  which needs h^2 = dx^2 + dy^2 instead of the fp64 square root (~30 instructions of the ~48 this test took; it runs for 20 cell pairs per column pair).
//  dx^2, dy^2, dz^2 are exact in fp64 (24-bit factors), the other products round at 1e-16: the 1e-9 band around zero still belongs to the reference expression.)
// 1 = ground, 0 = not ground, -1 = the margins cannot decide (within 1e-9 of a bound, or the shortcut is disabled: NaN tans)
IP_PRED_FN int ip_ground_margins(double tan_lo, double tan_hi, float fx, float fy, float fz) {
  const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
  const double h2 = dx * dx + dy * dy, z2 = dz * dz;
  const double l2 = (tan_lo * tan_lo) * h2, u2 = (tan_hi * tan_hi) * h2;   // (tan h)^2 of the two bounds
  const double sz = copysign(z2, dz);
  const double m1 = sz - copysign(l2, tan_lo), m2 = copysign(u2, tan_hi) - sz;
  const double t1 = 1e-9 * (z2 + l2), t2 = 1e-9 * (z2 + u2);
  const bool yes = m1 > t1 && m2 > t2, no = m1 < -t1 || m2 < -t2;
  return yes ? 1 : (no ? 0 : -1);
}
// the decision of ip_is_ground (ip_common.h) on the five numbers it takes from the handle
IP_PRED_FN bool ip_ground_decide(double tan_lo, double tan_hi, double mount, double thres, float fx, float fy, float fz) {
  const int g = ip_ground_margins(tan_lo, tan_hi, fx, fy, fz);
  if (g >= 0) return g != 0;
  return ip_is_ground_ref((double)fx, (double)fy, (double)fz, mount, thres);
}

// atan2(y, x) > theta for y > 0, x > 0 (y = d2 sin a, x = d1 - d2 cos a with d1 >= d2 > 0 and 0 < a < pi/2).
// tan is monotone on (0, pi/2): the comparison is decided by the sign of y - x tan(theta) whenever that difference is
// far (1e-9 relative) from zero — rounding errors of either form are ~1e-16 — and by the reference expression itself
// otherwise.  Saves two fp64 atan2 per cell on all but a vanishing fraction of the edges.
// the same decision without the reference expression: 1 / 0, or -1 when the margin cannot decide
IP_PRED_FN int edge_angle_margin(double y, double x, double tan_theta) {
  const double xt = x * tan_theta, m = y - xt;
  return fabs(m) > 1e-9 * (y + fabs(xt)) ? (m > 0.0 ? 1 : 0) : -1;
}
IP_PRED_FN bool edge_angle_gt(double y, double x, double theta, double tan_theta) {
  const double xt = x * tan_theta, m = y - xt;
  if (fabs(m) > 1e-9 * (y + fabs(xt))) return m > 0.0;
  return edge_angle_ref(y, x, theta);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The f32 screens.  Both decisions are signs; fp64 is needed only where the sign is in doubt.  A screen answers {yes, und}: und = it does not
// know (the caller evaluates the fp64 predicate for that site), otherwise yes IS the fp64 predicate's answer.  Every comparison is written so
// that NaN, inf, zero and denormal operands and the "disabled" constants (NaN / inf, ip_screen_consts) come out undecided.
struct IpScreenBits { bool yes, und; };

// Edge: y - x tan(theta) = tan(theta) (d2 K - d1) with K = (sin a + cos a tan(theta)) / tan(theta), so for tan(theta) > 0 the decision is the
// sign of E = d2 K - d1.  K is 1.002 / 1.020 at the default angles, in the densest part of neighbouring range ratios: a plain f32 product would
// leave one site in a thousand undecided.  K = kh + kl (two floats) and the product's rounding error e (an exact fma residual) give
//   E' = (p - d1) + (d2 kl + e),  p = fl(d2 kh):   |E' - E| <= 2^-23 |E'| + 2^-45 d1
// (p - d1 is exact when the two are within a factor of two, and a rounding error relative to |E| otherwise; the second bracket is 2^-22 p at
// most and rounds at 2^-24 of that; kh + kl misses K by 2^-48 K).  `band` (ip_edge_band) covers that, the 1e-9 band of edge_angle_gt and its
// fp64 roundings.  d2 below IP_SCREEN_TINY leaves the site undecided: the residual is exact only while d2 kh 2^-24 is a normal number.
#define IP_SCREEN_TINY 1e-24f
IP_PRED_FN IpScreenBits ip_edge_screen(float d1, float d2, float kh, float kl, float band) {
  const float p = d2 * kh, e = fmaf(d2, kh, -p), s = p - d1, E = s + fmaf(d2, kl, e);
  const bool dec = fabsf(E) > band * d1 && d2 >= IP_SCREEN_TINY;
  IpScreenBits r;
  r.yes = dec && E > 0.0f;
  r.und = !dec;
  return r;
}

// Ground: the signed-square margins of ip_ground_margins in f32.  g_lo / g_hi = sign(tan) tan^2 of the two bounds, g_max = max of the two
// squares.  f32 errors: h2 2^-23, z2 2^-24, the constants, the products and the differences 2^-24 each — under 4e-7 (z2 + g_max h2) in either
// margin, against a tolerance of 4e-6 of that sum (ten times the error, 4000 times the fp64 band).  Below IP_GROUND_FLOOR the squares are
// denormals and lose relative precision: undecided.
#define IP_GROUND_TOL 4e-6f
#define IP_GROUND_FLOOR 1e-30f
IP_PRED_FN IpScreenBits ip_ground_screen(float g_lo, float g_hi, float g_max, float fx, float fy, float fz) {
  const float h2 = fx * fx + fy * fy, z2 = fz * fz;
  const float sz = copysignf(z2, fz);
  const float m1 = sz - g_lo * h2, m2 = g_hi * h2 - sz;
  const float sum = z2 + g_max * h2, tol = IP_GROUND_TOL * sum;
  const bool big = sum >= IP_GROUND_FLOOR;
  const bool yes = m1 > tol && m2 > tol, no = m1 < -tol || m2 < -tol;
  IpScreenBits r;
  r.yes = yes && big;
  r.und = !((yes || no) && big);
  return r;
}

// The screens' constants, computed once per handle in fp64 (alego_create) and held in DevCtx.
struct IpScreenConsts {
  float kxh, kxl, kyh, kyl;   // K = kh + kl of seg_alpha_x / seg_alpha_y
  float eband;                // the edge screen decides when |E'| > eband d1; +inf: never
  float g_lo, g_hi, g_max;    // ground screen; NaN: never
};
// The edge band for one angle a, as a fraction of d1, or a negative number where the derivation does not hold.
//   A decided site has |E'| > band d1, hence |E| >= |E'| (1 - 2^-23) - 2^-45 d1.  The fp64 predicate computes m = y - x tan(theta) = tan(theta) E
//   with y = d2 sin a and |x tan(theta)| <= y + |m|, each of its four operations rounding at 2^-53 of operands that are at most
//   d1 (1 + tan(theta)): it decides, with the sign of E, when  tan(theta) |E| > 1e-9 (2 y + |m|) + 8 * 2^-53 d1 (1 + tan(theta)),  which follows
//   (d2 <= d1) from  |E| > [2.01e-9 sin a / tan(theta) + 1e-15 (1 + 1 / tan(theta))] d1.
//   band = 4 x (that bracket + 2^-45), and never below 8e-9: f32 cannot tell a smaller band from the rounding of band * d1 anyway.
// Premises: tan(theta) finite and > 0 (theta in (0, 1.5)), 0 < a < pi/2, K a normal float of moderate size, and a band that leaves the screen a use.
IP_PRED_HOST double ip_edge_band(double sin_a, double cos_a, double tan_theta) {
  if (!(tan_theta > 0.0) || !(tan_theta < 1e3) || !(sin_a > 0.0) || !(cos_a > 0.0) || !(sin_a < 1.0)) return -1.0;
  const double K = (sin_a + cos_a * tan_theta) / tan_theta;
  if (!(K > 1.0 / 1024.0) || !(K < 1024.0)) return -1.0;
  const double b = 4.0 * (2.01e-9 * sin_a / tan_theta + 1e-15 * (1.0 + 1.0 / tan_theta) + 2.9e-14);
  if (!(b < 1e-6)) return -1.0;
  return b > 8e-9 ? b : 8e-9;
}
// tan_theta / tan_lo / tan_hi as DevCtx holds them (NaN = that shortcut is disabled); enable = 0: every site undecided (ALEGO_IP_SCREEN=0)
IP_PRED_HOST IpScreenConsts ip_screen_consts(double sin_ax, double cos_ax, double sin_ay, double cos_ay, double tan_theta, double tan_lo, double tan_hi, int enable) {
  IpScreenConsts c;
  c.kxh = c.kxl = c.kyh = c.kyl = NAN; c.eband = INFINITY;
  c.g_lo = c.g_hi = c.g_max = NAN;
  if (!enable) return c;
  const double bx = ip_edge_band(sin_ax, cos_ax, tan_theta), by = ip_edge_band(sin_ay, cos_ay, tan_theta);
  if (bx > 0.0 && by > 0.0) {
    const double Kx = (sin_ax + cos_ax * tan_theta) / tan_theta, Ky = (sin_ay + cos_ay * tan_theta) / tan_theta;
    c.kxh = (float)Kx; c.kxl = (float)(Kx - (double)c.kxh);
    c.kyh = (float)Ky; c.kyl = (float)(Ky - (double)c.kyh);
    c.eband = (float)((bx > by ? bx : by) * (1.0 + 1e-6));   // (the band's own rounding to f32 and that of band * d1)
  }
  if (tan_lo < tan_hi && fabs(tan_lo) < 1e3 && fabs(tan_hi) < 1e3) {   // (NaN tans fail the comparison)
    const double l2 = tan_lo * tan_lo, u2 = tan_hi * tan_hi;
    c.g_lo = (float)copysign(l2, tan_lo); c.g_hi = (float)copysign(u2, tan_hi);
    c.g_max = (float)((l2 > u2 ? l2 : u2) * (1.0 + 1e-6));
  }
  return c;
}

#endif
