// reg_cov_math.h — the covariance of LaserMapping's scan-to-map registration and its degeneracy, f64 throughout,
// shared by the device kernel (lm_regcov, kernels_lm.hip) and the host twin (alego_regcov_host); readable by a host compiler without the
// HIP runtime (tests/reg_cov_math/reg_cov_math_check.cpp compiles this header alone).
//
// Input: the 28 scalars accumulate_block (solve_rows.h) delivers at the solver's final point p = (x, y, z, roll, pitch, yaw): the upper
// triangle of H = J^T J (Huber-corrected as the solver forms it), J^T r, the cost 1/2 sum rho; the row counts; the resolved options.
//   tangent   xi = M dp, GTSAM's right perturbation x <- x Expmap(xi), rotation first:  M = [[0, E], [R^T, 0]],  R = Rz(yaw) Ry(pitch) Rx(roll),
//             E (droll, dpitch, dyaw) = the body-frame rotation vector.  N = M^-1 = [[0, R], [E^-1, 0]] in closed form, info = N^T H N.
//   eigen     cyclic Jacobi on the 6x6 info: rotations (p, q) with p < q by rows, at most RC_SWEEPS_MAX sweeps, left as soon as the squared
//             off-diagonal mass is <= RC_OFF_REL times the squared diagonal mass.  Every rotation is written per ENTRY (rc_rot_col,
//             rc_rot_row): the 36 lanes of the kernel and the two loops of the host run the same operations on the same operands.
//   order     eigenvalues ascending, ties by index (rc_rank): the order is a function of the matrix alone
//   cov       sigma2 V diag(1 / max(lambda_k, floor * lambda_max)) V^T, entry (i, j) as sum_k (V_ik V_jk) w_k in ascending k: the products
//             commute, so cov is symmetric to the last bit
// Status: 1 computed; 0 fewer than 7 rows; -3 |cos pitch| < RC_COS_PITCH_MIN (E is singular there, as the solver's own Euler parameterisation is);
// -2 an input or a result is not finite.  With a status other than 1 every double of the record is zero.  The first three guards and the order
// belong to rc_spectrum, the front this header shares with remap_math.h; rc_compute adds only the finite check of its own results.
#ifndef ALEGO_REG_COV_MATH_H_
#define ALEGO_REG_COV_MATH_H_
#include <math.h>

#if defined(__HIPCC__)
#define RC_FN __host__ __device__ inline
#define RC_UNROLL _Pragma("unroll")
#else
#define RC_FN inline
#define RC_UNROLL
#endif

#define RC_COS_PITCH_MIN 1e-6
#define RC_SWEEPS_MAX 30
#define RC_OFF_REL 1e-40
// the resolved options as RC_OPT_W doubles (what the kernel reads): sigma0, scale, eig_min, lambda_rel_floor, var_min[6], var_max[6]
enum { RC_SIGMA0 = 0, RC_SCALE = 1, RC_EIG_MIN = 2, RC_LAMBDA_FLOOR = 3, RC_VAR_MIN = 4, RC_VAR_MAX = 10, RC_OPT_W = 16 };
#define RC_DEFAULT_SIGMA0 0.02
#define RC_DEFAULT_SCALE 1.0
#define RC_DEFAULT_EIG_MIN 100.0          // LeGO-LOAM's eignThre
#define RC_DEFAULT_LAMBDA_FLOOR 1e-12
#define RC_DEFAULT_VAR_MAX 1.0

// raw: the 16 doubles alego_regcov_opts starts with (the RC_* order), or null; a field <= 0 takes its default (var_min: var_min_dflt).
// Returns 0, or -1 when a field is not finite or var_min[k] > var_max[k].
RC_FN int rc_resolve(const double* raw, const double* var_min_dflt, double* opt) {
  opt[RC_SIGMA0] = RC_DEFAULT_SIGMA0; opt[RC_SCALE] = RC_DEFAULT_SCALE; opt[RC_EIG_MIN] = RC_DEFAULT_EIG_MIN; opt[RC_LAMBDA_FLOOR] = RC_DEFAULT_LAMBDA_FLOOR;
  for (int k = 0; k < 6; ++k) { opt[RC_VAR_MIN + k] = var_min_dflt[k]; opt[RC_VAR_MAX + k] = RC_DEFAULT_VAR_MAX; }
  if (raw)
    for (int k = 0; k < RC_OPT_W; ++k) {
      if (!(fabs(raw[k]) <= 1.7976931348623157e308)) return -1;
      if (raw[k] > 0.0) opt[k] = raw[k];
    }
  for (int k = 0; k < 6; ++k) if (opt[RC_VAR_MIN + k] > opt[RC_VAR_MAX + k]) return -1;
  return 0;
}

// H(i, j) of the 21 upper-triangle scalars (row by row, as accumulate_block stores them)
RC_FN double rc_h(const double* acc, int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return acc[a * 6 - (a * (a - 1)) / 2 + (b - a)];
}
// the sines and cosines M and N are made of: t = (sin roll, cos roll, sin pitch, cos pitch, sin yaw, cos yaw)
RC_FN void rc_trig(const double* p, double* t) { t[0] = sin(p[3]); t[1] = cos(p[3]); t[2] = sin(p[4]); t[3] = cos(p[4]); t[4] = sin(p[5]); t[5] = cos(p[5]); }
// M (row-major 6x6): xi = M dp.  (rc_m_t / rc_minv_t: from rc_trig's six values — a solver kernel has them in LDS from its evaluation at p)
RC_FN void rc_m_t(const double* t, double* M) {
  const double sr = t[0], cr = t[1], sp = t[2], cp = t[3], sy = t[4], cy = t[5];
  const double R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, -sp, cp * sr, cp * cr};
  const double E[9] = {1.0, 0.0, -sp, 0.0, cr, sr * cp, 0.0, -sr, cr * cp};
RC_UNROLL
  for (int k = 0; k < 36; ++k) M[k] = 0.0;
RC_UNROLL
  for (int r = 0; r < 3; ++r)
RC_UNROLL
    for (int c = 0; c < 3; ++c) { M[r * 6 + 3 + c] = E[r * 3 + c]; M[(3 + r) * 6 + c] = R[c * 3 + r]; }
}
RC_FN void rc_m(const double* p, double* M) { double t[6]; rc_trig(p, t); rc_m_t(t, M); }
// N = M^-1 (row-major 6x6): dp = N xi
RC_FN void rc_minv_t(const double* t, double* N) {
  const double sr = t[0], cr = t[1], sp = t[2], cp = t[3], sy = t[4], cy = t[5];
  const double R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, -sp, cp * sr, cp * cr};
  const double Ei[9] = {1.0, sr * sp / cp, cr * sp / cp, 0.0, cr, -sr, 0.0, sr / cp, cr / cp};
RC_UNROLL
  for (int k = 0; k < 36; ++k) N[k] = 0.0;
RC_UNROLL
  for (int r = 0; r < 3; ++r)
RC_UNROLL
    for (int c = 0; c < 3; ++c) { N[r * 6 + 3 + c] = R[r * 3 + c]; N[(3 + r) * 6 + c] = Ei[r * 3 + c]; }
}
RC_FN void rc_minv(const double* p, double* N) { double t[6]; rc_trig(p, t); rc_minv_t(t, N); }
// info(i, j) = (N^T H N)(i, j); callers pass i <= j and mirror
RC_FN double rc_info_entry(const double* acc, const double* N, int i, int j) {
  double s = 0.0;
RC_UNROLL
  for (int a = 0; a < 6; ++a) {
    double t = 0.0;
RC_UNROLL
    for (int b = 0; b < 6; ++b) t += rc_h(acc, a, b) * N[b * 6 + j];
    s += N[a * 6 + i] * t;
  }
  return s;
}
// the rotation that annihilates A(p, q) (apq != 0)
RC_FN void rc_rot_cs(double app, double aqq, double apq, double* c, double* s) {
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  *c = 1.0 / sqrt(t * t + 1.0);
  *s = t * *c;
}
// X <- X G for the entry in column j: xp = X(i, p), xq = X(i, q) before the step
RC_FN double rc_rot_col(int j, int p, int q, double c, double s, double xp, double xq, double self) {
  return j == p ? c * xp - s * xq : (j == q ? s * xp + c * xq : self);
}
// X <- G^T X for the entry in row i: xp = X(p, j), xq = X(q, j) before the step
RC_FN double rc_rot_row(int i, int p, int q, double c, double s, double xp, double xq, double self) {
  return i == p ? c * xp - s * xq : (i == q ? s * xp + c * xq : self);
}
// position of d[k] in ascending order, ties by index
RC_FN int rc_rank(const double* d, int k) {
  int r = 0;
RC_UNROLL
  for (int m = 0; m < 6; ++m) r += (d[m] < d[k] || (d[m] == d[k] && m < k)) ? 1 : 0;
  return r;
}
RC_FN double rc_weight(double lam, double lam_max, double floor_rel) { const double f = floor_rel * lam_max; return 1.0 / (lam > f ? lam : f); }
// cov(i, j) / sigma2 from the sorted eigenvectors' rows i and j and the weights
RC_FN double rc_cov_entry(const double* vi, const double* vj, const double* w) {
  double s = 0.0;
RC_UNROLL
  for (int k = 0; k < 6; ++k) s += (vi[k] * vj[k]) * w[k];
  return s;
}
RC_FN double rc_sigma2(double cost, int rows, double sigma0) { const double a = sigma0 * sigma0, b = 2.0 * cost / (double)(rows - 6); return b > a ? b : a; }
RC_FN double rc_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
RC_FN bool rc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// The cyclic Jacobi of a symmetric 6x6 A (row-major, overwritten: its diagonal ends as the eigenvalues) with V <- V G for every rotation G
// (V = I on entry: the eigenvectors by columns).  *sweeps (optional) is advanced by the sweeps in which a rotation was made.  The one loop of the
// host twins (rc_spectrum); the kernels run the same rotations entry by entry on 36 lanes.
RC_FN void rc_jacobi(double* A, double* V, int* sweeps) {
  double B[36];
  for (int sweep = 0; sweep < RC_SWEEPS_MAX; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int i = 0; i < 6; ++i)
      for (int j = i + 1; j < 6; ++j) off += A[i * 6 + j] * A[i * 6 + j];
    for (int i = 0; i < 6; ++i) dg += A[i * 6 + i] * A[i * 6 + i];
    if (!(off > RC_OFF_REL * dg)) break;
    if (sweeps) *sweeps += 1;
    for (int pp = 0; pp < 5; ++pp)
      for (int q = pp + 1; q < 6; ++q) {
        const double apq = A[pp * 6 + q];
        if (apq == 0.0) continue;
        double c, s;
        rc_rot_cs(A[pp * 6 + pp], A[q * 6 + q], apq, &c, &s);
        for (int k = 0; k < 36; ++k) B[k] = A[k];
        for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) A[i * 6 + j] = rc_rot_col(j, pp, q, c, s, B[i * 6 + pp], B[i * 6 + q], B[i * 6 + j]);
        for (int k = 0; k < 36; ++k) B[k] = A[k];
        for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) A[i * 6 + j] = rc_rot_row(i, pp, q, c, s, B[pp * 6 + j], B[q * 6 + j], B[i * 6 + j]);
        for (int k = 0; k < 36; ++k) B[k] = V[k];
        for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) V[i * 6 + j] = rc_rot_col(j, pp, q, c, s, B[i * 6 + pp], B[i * 6 + q], B[i * 6 + j]);
      }
  }
}
// ... and its result in ascending order, ties by index: lam[r] and column r of Vs from the diagonal entry of rank r
RC_FN void rc_sort(const double* A, const double* V, double* lam, double* Vs) {
  double d[6];
  for (int k = 0; k < 6; ++k) d[k] = A[k * 6 + k];
  for (int k = 0; k < 6; ++k) { const int r = rc_rank(d, k); lam[r] = d[k]; for (int i = 0; i < 6; ++i) Vs[i * 6 + r] = V[i * 6 + k]; }
}

// The spectrum of a registration: the one front of the host twins (rc_compute; rm_compute, remap_math.h) and the owner of their guards, in this order:
// fewer than 7 rows -> 0; |cos pitch| < RC_COS_PITCH_MIN -> -3; an input or an entry of info not finite -> -2; else 1 with N = M(p)^-1, the unrotated
// info = N^T H N, lam[6] ascending and the eigenvectors Vs sorted likewise (nothing is to be read with another status).  *sweeps (optional, zeroed by the
// caller) is advanced by the sweeps in which a rotation was made.  The kernels run the same, entry by entry, in rc_front_lanes (kernels_lm.hip).
RC_FN int rc_spectrum(const double* acc, const double* p, int n_edge, int n_plane, double* N, double* info, double* lam, double* Vs, int* sweeps) {
  if (n_edge + n_plane <= 6) return 0;
  if (fabs(cos(p[4])) < RC_COS_PITCH_MIN) return -3;
  bool bad = false;
  for (int k = 0; k < 28; ++k) bad = bad || !rc_finite(acc[k]);
  for (int k = 0; k < 6; ++k) bad = bad || !rc_finite(p[k]);
  double A[36], V[36];
  rc_minv(p, N);
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { const double v = rc_info_entry(acc, N, i, j); A[i * 6 + j] = v; A[j * 6 + i] = v; }
  for (int k = 0; k < 36; ++k) { bad = bad || !rc_finite(A[k]); V[k] = (k % 7 == 0) ? 1.0 : 0.0; }
  if (bad) return -2;
  for (int k = 0; k < 36; ++k) info[k] = A[k];
  rc_jacobi(A, V, sweeps);
  rc_sort(A, V, lam, Vs);
  return 1;
}

// The record as plain arrays (the host twin; the kernel does the same entry by entry on 36 lanes): the covariance tail of rc_spectrum.  Returns the
// status; *sweeps (optional): sweeps in which a rotation was made.
RC_FN int rc_compute(const double* acc, const double* p, int n_edge, int n_plane, const double* opt, double* sigma2, double* info, double* eigval, double* eigvec,
                     double* cov, double* variance, int* n_degenerate, int* sweeps) {
  *sigma2 = 0.0; *n_degenerate = 0;
  if (sweeps) *sweeps = 0;
  for (int k = 0; k < 36; ++k) { info[k] = 0.0; eigvec[k] = 0.0; cov[k] = 0.0; }
  for (int k = 0; k < 6; ++k) { eigval[k] = 0.0; variance[k] = 0.0; }
  double N[36], inf0[36], lam[6], Vs[36], w[6], cv[36];
  const int st = rc_spectrum(acc, p, n_edge, n_plane, N, inf0, lam, Vs, sweeps);
  if (st != 1) return st;
  const double s2 = rc_sigma2(acc[27], n_edge + n_plane, opt[RC_SIGMA0]);
  for (int k = 0; k < 6; ++k) w[k] = rc_weight(lam[k], lam[5], opt[RC_LAMBDA_FLOOR]);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) cv[i * 6 + j] = s2 * rc_cov_entry(Vs + i * 6, Vs + j * 6, w);
  bool bad = !rc_finite(s2);
  for (int k = 0; k < 36; ++k) bad = bad || !rc_finite(Vs[k]) || !rc_finite(cv[k]);
  for (int k = 0; k < 6; ++k) bad = bad || !rc_finite(lam[k]);
  if (bad) return -2;
  *sigma2 = s2;
  for (int k = 0; k < 36; ++k) { info[k] = inf0[k]; eigvec[k] = Vs[k]; cov[k] = cv[k]; }
  for (int k = 0; k < 6; ++k) {
    eigval[k] = lam[k];
    *n_degenerate += lam[k] < opt[RC_EIG_MIN] ? 1 : 0;
    variance[k] = rc_clamp(opt[RC_SCALE] * cv[k * 6 + k], opt[RC_VAR_MIN + k], opt[RC_VAR_MAX + k]);
  }
  return 1;
}

#endif
