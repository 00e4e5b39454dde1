// csrc/reg_cov_math.h on the host, compiled alone (no HIP runtime) with AddressSanitizer and UBSan by tests/test_reg_cov_math.py.
//   1. M against finite differences of pg_math.h's Logmap: M dp = Logmap(x(p)^-1 x(p + dp)) to the second-order term
//   2. rc_compute on constructed normal equations: H V = V Lambda, V^T V = I, ascending order, symmetric cov, every status, every clamp
//      on both sides of its bound, the options' defaults
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pg_math.h"
#include "reg_cov_math.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void pose_of(const double* p, double* X) {
  double R[9];
  pg_rzryrx(p[3], p[4], p[5], R);
  for (int r = 0; r < 3; ++r) { X[r * 4 + 0] = R[r * 3 + 0]; X[r * 4 + 1] = R[r * 3 + 1]; X[r * 4 + 2] = R[r * 3 + 2]; X[r * 4 + 3] = p[r]; }
}

static double check_m() {
  const double poses[][6] = {
      {0, 0, 0, 0, 0, 0},          {1.5, -2.0, 0.3, 0.1, -0.2, 0.3},   {10, 20, -3, 0.4, 1.2, -2.0},    {-7, 4, 1, -0.7, -1.2, 3.0},
      {3, 3, 3, 2.5, 1.19, 3.14159}, {3, 3, 3, -2.5, -1.21, -3.14159}, {0.1, 0.2, 0.3, 3.1, 0.05, 3.1415926}, {100, -50, 2, 0.01, 0.02, -3.1415926},
  };
  const double delta = 1e-6;
  double worst = 0.0;
  for (const auto& p : poses) {
    double M[36], N[36], X0[12];
    rc_m(p, M);
    rc_minv(p, N);
    pose_of(p, X0);
    for (int i = 0; i < 6; ++i)   // N is M's inverse
      for (int j = 0; j < 6; ++j) {
        double s = 0;
        for (int k = 0; k < 6; ++k) s += M[i * 6 + k] * N[k * 6 + j];
        CHECK(std::fabs(s - (i == j ? 1.0 : 0.0)) < 1e-13, "M N (%d, %d) = %.17g at pitch %g", i, j, s, p[4]);
      }
    for (int k = 0; k < 6; ++k) {
      double q[6], X1[12], B[12], xi[6];
      for (int c = 0; c < 6; ++c) q[c] = p[c];
      q[k] += delta;
      // (yaw beyond +-pi is the same rotation: the perturbed pose needs no wrapping)
      pose_of(q, X1);
      pg_between(X0, X1, B);
      pg_log(B, xi);
      for (int r = 0; r < 6; ++r) {
        const double e = std::fabs(xi[r] - M[r * 6 + k] * delta);
        if (e > worst) worst = e;
        CHECK(e <= 1e-10, "M column %d row %d: Logmap %.17g, M dp %.17g (pitch %g yaw %g)", k, r, xi[r], M[r * 6 + k] * delta, p[4], p[5]);
      }
    }
  }
  return worst;
}

// a fixed orthogonal matrix: the product of Givens rotations over all pairs with angles 0.3 + 0.37 (p + 2 q)
static void ortho(double* Q) {
  for (int k = 0; k < 36; ++k) Q[k] = (k % 7 == 0) ? 1.0 : 0.0;
  for (int p = 0; p < 5; ++p)
    for (int q = p + 1; q < 6; ++q) {
      const double a = 0.3 + 0.37 * (p + 2 * q), c = std::cos(a), s = std::sin(a);
      for (int r = 0; r < 6; ++r) { const double xp = Q[r * 6 + p], xq = Q[r * 6 + q]; Q[r * 6 + p] = c * xp - s * xq; Q[r * 6 + q] = s * xp + c * xq; }
    }
}
static void acc_of(const double* H, double cost, double* acc) {
  int t = 0;
  for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) acc[t++] = 0.5 * (H[i * 6 + j] + H[j * 6 + i]);
  for (int k = 0; k < 6; ++k) acc[21 + k] = 0.0;
  acc[27] = cost;
}
static void spd(const double* lam, bool rotate, double* H) {
  double Q[36];
  ortho(Q);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double s = 0;
      if (rotate) for (int k = 0; k < 6; ++k) s += Q[i * 6 + k] * lam[k] * Q[j * 6 + k];
      else s = i == j ? lam[i] : 0.0;
      H[i * 6 + j] = s;
    }
}

struct Rec { double sigma2, info[36], eigval[6], eigvec[36], cov[36], variance[6]; int ndeg, sweeps, status; };
static Rec run(const double* acc, const double* p, int ne, int np, const double* opt) {
  Rec r;
  r.status = rc_compute(acc, p, ne, np, opt, &r.sigma2, r.info, r.eigval, r.eigvec, r.cov, r.variance, &r.ndeg, &r.sweeps);
  return r;
}
static bool all_zero(const Rec& r) {
  bool z = r.sigma2 == 0.0 && r.ndeg == 0;
  for (int k = 0; k < 36; ++k) z = z && r.info[k] == 0.0 && r.eigvec[k] == 0.0 && r.cov[k] == 0.0;
  for (int k = 0; k < 6; ++k) z = z && r.eigval[k] == 0.0 && r.variance[k] == 0.0;
  return z;
}

static void check_decomposition(double* worst_res, double* worst_orth, int* worst_sweeps) {
  const double dflt_min[6] = {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6};
  double opt[RC_OPT_W];
  CHECK(rc_resolve(nullptr, dflt_min, opt) == 0, "defaults");
  const double sets[][6] = {
      {1, 1, 1, 1, 1, 1},                    // condition 1, six equal eigenvalues
      {1, 2, 3, 4, 5, 6},
      {1e3, 2e3, 5e3, 1e4, 5e4, 1e6},        // condition 1e3
      {1, 1e1, 1e2, 1e4, 1e5, 1e6},          // 1e6
      {1e-3, 1, 10, 1e3, 1e6, 1e9},          // 1e12
      {5, 5, 5, 700, 700, 3000},             // repeated
      {0, 0, 0, 10, 200, 4000},              // rank 3
      {0, 3, 30, 300, 3000, 30000},          // rank 5
  };
  const double poses[][6] = {{0, 0, 0, 0, 0, 0}, {4, -3, 1, 0.3, -0.4, 2.9}, {1, 2, 3, -1.0, 1.2, -3.1}};
  for (const auto& lam : sets)
    for (int rotate = 0; rotate < 2; ++rotate)
      for (const auto& p : poses) {
        double H[36], acc[28];
        spd(lam, rotate != 0, H);
        acc_of(H, 0.5 * 1000 * 0.01, acc);   // cost of 1000 rows with residual variance 0.01
        const Rec r = run(acc, p, 400, 600, opt);
        CHECK(r.status == 1, "status %d", r.status);
        if (r.status != 1) continue;
        if (r.sweeps > *worst_sweeps) *worst_sweeps = r.sweeps;
        CHECK(r.sweeps < RC_SWEEPS_MAX, "Jacobi did not converge in %d sweeps", r.sweeps);
        // info = N^T H N, recomputed plainly
        double N[36];
        rc_minv(p, N);
        const double lmax = r.eigval[5];
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j) {
            double s = 0;
            for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) s += N[a * 6 + i] * H[a * 6 + b] * N[b * 6 + j];
            CHECK(std::fabs(s - r.info[i * 6 + j]) <= 1e-13 * lmax, "info (%d, %d)", i, j);
            CHECK(r.info[i * 6 + j] == r.info[j * 6 + i], "info is symmetric");
          }
        for (int k = 0; k + 1 < 6; ++k) CHECK(r.eigval[k] <= r.eigval[k + 1], "ascending: %g > %g", r.eigval[k], r.eigval[k + 1]);
        for (int i = 0; i < 6; ++i)
          for (int k = 0; k < 6; ++k) {
            double hv = 0, vv = 0;
            for (int a = 0; a < 6; ++a) { hv += r.info[i * 6 + a] * r.eigvec[a * 6 + k]; vv += r.eigvec[a * 6 + i] * r.eigvec[a * 6 + k]; }
            const double res = std::fabs(hv - r.eigvec[i * 6 + k] * r.eigval[k]) / lmax, orth = std::fabs(vv - (i == k ? 1.0 : 0.0));
            if (res > *worst_res) *worst_res = res;
            if (orth > *worst_orth) *worst_orth = orth;
            CHECK(res <= 1e-13, "H V = V Lambda: (%d, %d) off by %g of lambda_max", i, k, res);
            CHECK(orth <= 1e-14, "V^T V = I: (%d, %d) off by %g", i, k, orth);
          }
        // eigenvalues against the construction (similar matrices at p = 0: N is a permutation there)
        if (p[3] == 0.0 && p[4] == 0.0 && p[5] == 0.0) {
          double s[6];
          for (int k = 0; k < 6; ++k) s[k] = lam[k];
          for (int a = 0; a < 6; ++a) for (int b = a + 1; b < 6; ++b) if (s[b] < s[a]) { const double t = s[a]; s[a] = s[b]; s[b] = t; }
          for (int k = 0; k < 6; ++k) CHECK(std::fabs(r.eigval[k] - s[k]) <= 1e-13 * lmax, "eigenvalue %d: %.17g, built with %.17g", k, r.eigval[k], s[k]);
          int nd = 0;
          for (int k = 0; k < 6; ++k) nd += r.eigval[k] < opt[RC_EIG_MIN] ? 1 : 0;
          CHECK(r.ndeg == nd, "n_degenerate %d, counted %d", r.ndeg, nd);
        }
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j) CHECK(std::memcmp(&r.cov[i * 6 + j], &r.cov[j * 6 + i], sizeof(double)) == 0, "cov is symmetric to the last bit");
        CHECK(r.sigma2 == rc_sigma2(acc[27], 1000, opt[RC_SIGMA0]) && std::fabs(r.sigma2 - 0.01 * 1000.0 / 994.0) < 1e-15, "sigma2 %.17g", r.sigma2);
        // cov = sigma2 V diag(w) V^T with the floored weights
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j) {
            double s = 0, big = 0;
            for (int k = 0; k < 6; ++k) {
              const double f = opt[RC_LAMBDA_FLOOR] * lmax, w = 1.0 / (r.eigval[k] > f ? r.eigval[k] : f);
              s += r.eigvec[i * 6 + k] * w * r.eigvec[j * 6 + k];
              big += std::fabs(r.eigvec[i * 6 + k] * w * r.eigvec[j * 6 + k]);
            }
            CHECK(std::fabs(r.sigma2 * s - r.cov[i * 6 + j]) <= 1e-14 * r.sigma2 * big, "cov (%d, %d)", i, j);
          }
        for (int k = 0; k < 6; ++k) CHECK(r.variance[k] == rc_clamp(opt[RC_SCALE] * r.cov[k * 6 + k], opt[RC_VAR_MIN + k], opt[RC_VAR_MAX + k]), "variance %d", k);
      }
}

static void check_status_and_clamps() {
  const double dflt_min[6] = {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6};
  double opt[RC_OPT_W];
  rc_resolve(nullptr, dflt_min, opt);
  CHECK(opt[RC_SIGMA0] == 0.02 && opt[RC_SCALE] == 1.0 && opt[RC_EIG_MIN] == 100.0 && opt[RC_LAMBDA_FLOOR] == 1e-12, "defaults");
  for (int k = 0; k < 6; ++k) CHECK(opt[RC_VAR_MIN + k] == dflt_min[k] && opt[RC_VAR_MAX + k] == 1.0, "default bounds");
  double raw[RC_OPT_W] = {0.05, -1.0, 0.0, 1e-9, 1e-4, 0, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0}, o2[RC_OPT_W];
  CHECK(rc_resolve(raw, dflt_min, o2) == 0 && o2[RC_SIGMA0] == 0.05 && o2[RC_SCALE] == 1.0 && o2[RC_EIG_MIN] == 100.0 && o2[RC_LAMBDA_FLOOR] == 1e-9 &&
        o2[RC_VAR_MIN] == 1e-4 && o2[RC_VAR_MIN + 1] == 1e-6 && o2[RC_VAR_MAX] == 0.5 && o2[RC_VAR_MAX + 1] == 1.0, "fields <= 0 take their defaults");
  raw[RC_VAR_MIN + 2] = 2.0;   // above var_max[2] = 1
  CHECK(rc_resolve(raw, dflt_min, o2) == -1, "var_min > var_max");
  raw[RC_VAR_MIN + 2] = 1.0;   // equal is allowed
  CHECK(rc_resolve(raw, dflt_min, o2) == 0, "var_min == var_max");
  raw[RC_SCALE] = std::numeric_limits<double>::quiet_NaN();
  CHECK(rc_resolve(raw, dflt_min, o2) == -1, "NaN option");
  raw[RC_SCALE] = std::numeric_limits<double>::infinity();
  CHECK(rc_resolve(raw, dflt_min, o2) == -1, "infinite option");

  const double lam[6] = {200, 300, 400, 500, 600, 700}, zero6[6] = {0, 0, 0, 0, 0, 0};
  double H[36], acc[28];
  spd(lam, true, H);
  acc_of(H, 1.0, acc);
  const double p0[6] = {1, 2, 3, 0.1, 0.2, 0.3};
  // row counts
  Rec r = run(acc, p0, 3, 3, opt);
  CHECK(r.status == 0 && all_zero(r), "6 rows: status %d", r.status);
  r = run(acc, p0, 0, 0, opt);
  CHECK(r.status == 0 && all_zero(r), "no rows: status %d", r.status);
  r = run(acc, p0, 3, 4, opt);
  CHECK(r.status == 1 && r.sigma2 == 2.0, "7 rows: status %d sigma2 %g", r.status, r.sigma2);
  r = run(acc, p0, 7, 0, opt);
  CHECK(r.status == 1, "7 edge rows: status %d", r.status);
  // pitch
  double pp[6] = {1, 2, 3, 0.1, std::acos(-1.0) / 2, 0.3};
  r = run(acc, pp, 10, 10, opt);
  CHECK(r.status == -3 && all_zero(r), "pitch pi/2: status %d", r.status);
  pp[4] = std::acos(0.5e-6);
  r = run(acc, pp, 10, 10, opt);
  CHECK(r.status == -3, "cos pitch 0.5e-6: status %d", r.status);
  pp[4] = -std::acos(2e-6);
  r = run(acc, pp, 10, 10, opt);
  CHECK(r.status == 1, "cos pitch 2e-6: status %d", r.status);
  // not finite
  for (int k : {0, 20, 21, 27}) {
    double bad[28];
    std::memcpy(bad, acc, sizeof(bad));
    bad[k] = k == 20 ? std::numeric_limits<double>::infinity() : std::numeric_limits<double>::quiet_NaN();
    r = run(bad, p0, 10, 10, opt);
    CHECK(r.status == -2 && all_zero(r), "scalar %d not finite: status %d", k, r.status);
  }
  for (int k = 0; k < 6; ++k) {
    double q[6];
    std::memcpy(q, p0, sizeof(q));
    q[k] = std::numeric_limits<double>::quiet_NaN();
    r = run(acc, q, 10, 10, opt);
    CHECK(r.status == -2 && all_zero(r), "parameter %d not finite: status %d", k, r.status);
  }
  spd(zero6, false, H);   // the zero matrix: lambda_max = 0, no weight is finite
  acc_of(H, 1.0, acc);
  r = run(acc, p0, 10, 10, opt);
  CHECK(r.status == -2 && all_zero(r), "zero matrix: status %d", r.status);
  // a diagonal matrix at p = 0: info is H with (translation, rotation) swapped, cov = sigma2 / h, eigenvectors the unit vectors
  const double h[6] = {4000, 50, 600, 70000, 800, 9};   // x y z roll pitch yaw
  const double pz[6] = {0, 0, 0, 0, 0, 0};
  spd(h, false, H);
  acc_of(H, 0.5 * 94 * 0.25, acc);   // 100 rows: sigma2 = 0.25
  double wide[RC_OPT_W];
  std::memcpy(wide, opt, sizeof(wide));
  for (int k = 0; k < 6; ++k) { wide[RC_VAR_MIN + k] = 1e-300; wide[RC_VAR_MAX + k] = 1e300; }
  r = run(acc, pz, 40, 60, wide);
  CHECK(r.status == 1 && r.sigma2 == 0.25 && r.sweeps == 0, "diagonal: status %d sigma2 %g sweeps %d", r.status, r.sigma2, r.sweeps);
  const double want_tan[6] = {h[3], h[4], h[5], h[0], h[1], h[2]};
  for (int k = 0; k < 6; ++k) {
    CHECK(r.info[k * 6 + k] == want_tan[k], "info diag %d = %g", k, r.info[k * 6 + k]);
    CHECK(r.variance[k] == 0.25 / want_tan[k], "variance %d = %.17g", k, r.variance[k]);
  }
  CHECK(r.eigval[0] == 9 && r.eigval[5] == 70000 && r.ndeg == 2, "sorted %g .. %g, %d below eig_min", r.eigval[0], r.eigval[5], r.ndeg);
  CHECK(r.eigvec[2 * 6 + 0] == 1.0 && r.eigvec[0 * 6 + 5] == 1.0, "eigenvector of the smallest eigenvalue (yaw's) is rotation z, of the largest (roll's) rotation x");
  // ties keep their index order
  const double tie[6] = {7, 7, 7, 7, 7, 7};
  spd(tie, false, H);
  acc_of(H, 1.0, acc);
  r = run(acc, pz, 40, 60, wide);
  for (int k = 0; k < 36; ++k) CHECK(r.eigvec[k] == ((k % 7 == 0) ? 1.0 : 0.0), "ties by index: eigvec[%d] = %g", k, r.eigvec[k]);
  // every clamp on both sides of its bound, and scale
  spd(h, false, H);
  acc_of(H, 0.5 * 94 * 0.25, acc);
  for (int k = 0; k < 6; ++k) {
    const double v = 0.25 / want_tan[k];
    double o[RC_OPT_W];
    std::memcpy(o, wide, sizeof(o));
    o[RC_VAR_MIN + k] = v * (1 + 1e-12);
    CHECK(run(acc, pz, 40, 60, o).variance[k] == o[RC_VAR_MIN + k], "below var_min[%d]: raised", k);
    o[RC_VAR_MIN + k] = v * (1 - 1e-12);
    CHECK(run(acc, pz, 40, 60, o).variance[k] == v, "above var_min[%d]: kept", k);
    o[RC_VAR_MIN + k] = 1e-300;
    o[RC_VAR_MAX + k] = v * (1 - 1e-12);
    CHECK(run(acc, pz, 40, 60, o).variance[k] == o[RC_VAR_MAX + k], "above var_max[%d]: lowered", k);
    o[RC_VAR_MAX + k] = v * (1 + 1e-12);
    CHECK(run(acc, pz, 40, 60, o).variance[k] == v, "below var_max[%d]: kept", k);
    o[RC_SCALE] = 3.0;
    o[RC_VAR_MAX + k] = 1e300;
    CHECK(run(acc, pz, 40, 60, o).variance[k] == 3.0 * v, "scale");
  }
  // sigma0 floors sigma2; eig_min counts; the relative floor bounds the weight of a null direction
  acc_of(H, 0.0, acc);
  r = run(acc, pz, 40, 60, wide);
  CHECK(r.sigma2 == 0.02 * 0.02, "sigma0 floor: %g", r.sigma2);
  double o[RC_OPT_W];
  std::memcpy(o, wide, sizeof(o));
  o[RC_EIG_MIN] = 700;
  CHECK(run(acc, pz, 40, 60, o).ndeg == 3, "eig_min 700");
  const double nul[6] = {0, 50, 600, 70000, 800, 9};
  spd(nul, false, H);
  acc_of(H, 0.5 * 94 * 0.25, acc);
  r = run(acc, pz, 40, 60, wide);
  CHECK(r.status == 1 && r.variance[3] == 0.25 * (1.0 / (1e-12 * 70000)), "null direction: variance %g", r.variance[3]);
}

int main() {
  const double fd = check_m();
  double res = 0, orth = 0;
  int sweeps = 0;
  check_decomposition(&res, &orth, &sweeps);
  check_status_and_clamps();
  std::printf("largest |Logmap - M dp| %.3g; largest residual %.3g of lambda_max, largest |V^T V - I| %.3g, most sweeps %d\n", fd, res, orth, sweeps);
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("reg_cov_math ok\n");
  return 0;
}
