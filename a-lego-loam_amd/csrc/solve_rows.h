// solve_rows.h — the four analytic-Jacobian cost functors of include/alego/utility.h:122-349 with the small Eigen-equivalent rotation helpers
// they need, and the trust-region control of the two solvers (lo_solve_t, lm_solve; lm_shard_step).  Readable by a host compiler without the HIP
// runtime: tests/solve_rows/solve_rows_check.cpp runs the cost-first control against the full evaluation of every point on the CPU.
#ifndef ALEGO_SOLVE_ROWS_H_
#define ALEGO_SOLVE_ROWS_H_

#ifdef __HIPCC__
#define SOLVE_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define SOLVE_FN inline
#endif
#include "remap_math.h"
#ifdef __HIP_DEVICE_COMPILE__
#define SOLVE_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define SOLVE_SCHED_FENCE() ((void)0)
#endif

// The candidate policy of lo_solve_t and lm_solve, one definition for both.  1: the candidate after a successful step is evaluated in full at once
// (it is adopted more often than not, and adopting it then costs no second pass); 0: every candidate for its cost first.  The results are the same
// either way; 1 issues fewer VALU instructions over lm_solve + lo_solve_t together and measured faster (profiles/r08_solver_eval.md).
#ifndef ALEGO_SOLVE_SPECULATE
#define ALEGO_SOLVE_SPECULATE 1
#endif

enum { BLK_SURF = 0, BLK_CORNER = 1, BLK_EDGE = 2, BLK_PLANE = 3 };

struct DQuat { double w, x, y, z; };

SOLVE_FN DQuat dq_mul(const DQuat& a, const DQuat& b) {
  DQuat r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
  return r;
}
// AngleAxisd(yaw,Z) * AngleAxisd(pitch,Y) * AngleAxisd(roll,X)  (utility.h:128, laserOdometry.cpp:731)
SOLVE_FN DQuat dq_zyx(double yaw, double pitch, double roll) {
  const double hz = 0.5 * yaw, hy = 0.5 * pitch, hx = 0.5 * roll;
  DQuat qz{cos(hz), 0, 0, sin(hz)}, qy{cos(hy), 0, sin(hy), 0}, qx{cos(hx), sin(hx), 0, 0};
  return dq_mul(dq_mul(qz, qy), qx);
}
SOLVE_FN void dq_rotate(const DQuat& q, const double v[3], double out[3]) {
  const double u0 = 2 * (q.y * v[2] - q.z * v[1]), u1 = 2 * (q.z * v[0] - q.x * v[2]), u2 = 2 * (q.x * v[1] - q.y * v[0]);
  out[0] = v[0] + q.w * u0 + (q.y * u2 - q.z * u1);
  out[1] = v[1] + q.w * u1 + (q.z * u0 - q.x * u2);
  out[2] = v[2] + q.w * u2 + (q.x * u1 - q.y * u0);
}
// Pose-dependent terms shared by every residual of one evaluation.
struct PoseTerms {
  DQuat q;
  double t[3];
  double sr, cr, sp, cp, sy, cy;
};
SOLVE_FN PoseTerms pose_terms(const double* p) {
  PoseTerms T;
  T.q = dq_zyx(p[5], p[4], p[3]);
  T.t[0] = p[0]; T.t[1] = p[1]; T.t[2] = p[2];
  T.sr = sin(p[3]); T.cr = cos(p[3]); T.sp = sin(p[4]); T.cp = cos(p[4]); T.sy = sin(p[5]); T.cy = cos(p[5]);
  return T;
}

// residual + 1x6 Jacobian (uncorrected).  a = lpj | plane normal, b = lpl, c = lpm, dd = negative_OA_dot_norm.
SOLVE_FN void eval_block(int type, const double cp_[3], const double a[3], const double b[3], const double c[3], double dd,
                           const PoseTerms& T, double* res, double J[6]) {
  double lp[3];
  dq_rotate(T.q, cp_, lp);
  lp[0] += T.t[0]; lp[1] += T.t[1]; lp[2] += T.t[2];
  const double X = cp_[0], Y = cp_[1], Z = cp_[2];
  const double sr = T.sr, cr = T.cr, sp = T.sp, cp = T.cp, sy = T.sy, cy = T.cy;
  if (type == BLK_SURF) {  // utility.h:185-235
    double ca = (a[1] - b[1]) * (a[2] - c[2]) - (a[2] - b[2]) * (a[1] - c[1]);
    double cb = (a[2] - b[2]) * (a[0] - c[0]) - (a[0] - b[0]) * (a[2] - c[2]);
    double cc = (a[0] - b[0]) * (a[1] - c[1]) - (a[1] - b[1]) * (a[0] - c[0]);
    ca *= ca; cb *= cb; cc *= cc;
    const double ex = lp[0] - a[0], ey = lp[1] - a[1], ez = lp[2] - a[2];
    const double m = sqrt(ex * ex * ca + ey * ey * cb + ez * ez * cc);
    const double k = sqrt(ca + cb + cc);
    *res = m / k;
    const double tmp = m * k;
    J[0] = 0.; J[1] = 0.; J[2] = ((ez * cc) / tmp) / k; J[3] = 0.; J[4] = 0.; J[5] = 0.;
    return;
  }
  // shared derivative table utility.h:148-158 (dy_dp keeps the reference's cr*sr*cp term)
  const double dx_dr = (cy * sp * cr + sr * sy) * Y + (sy * cr - cy * sr * sp) * Z;
  const double dy_dr = (-cy * sr + sy * sp * cr) * Y + (-sr * sy * sp - cy * cr) * Z;
  const double dz_dr = cp * cr * Y - cp * sr * Z;
  const double dx_dp = -cy * sp * X + cy * cp * sr * Y + cy * cr * cp * Z;
  const double dy_dp = -sp * sy * X + sy * cp * sr * Y + cr * sr * cp * Z;
  const double dz_dp = -cp * X - sp * sr * Y - sp * cr * Z;
  const double dx_dy = -sy * cp * X - (sy * sp * sr + cr * cy) * Y + (cy * sr - sy * cr * sp) * Z;
  const double dy_dy = cp * cy * X + (-sy * cr + cy * sp * sr) * Y + (cy * cr * sp + sy * sr) * Z;
  const double dz_dy = 0.;
  if (type == BLK_PLANE) {  // utility.h:307-343
    *res = (a[0] * lp[0] + a[1] * lp[1] + a[2] * lp[2]) + dd;
    J[0] = a[0]; J[1] = a[1]; J[2] = a[2];
    J[3] = a[0] * dx_dr + a[1] * dy_dr + a[2] * dz_dr;
    J[4] = a[0] * dx_dp + a[1] * dy_dp + a[2] * dz_dp;
    J[5] = a[0] * dx_dy + a[1] * dy_dy + a[2] * dz_dy;
    return;
  }
  // BLK_CORNER utility.h:126-174 / BLK_EDGE utility.h:246-294
  const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
  const double k = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  const double ca = (lp[1] - a[1]) * (lp[2] - b[2]) - (lp[2] - a[2]) * (lp[1] - b[1]);
  const double cb = (lp[2] - a[2]) * (lp[0] - b[0]) - (lp[0] - a[0]) * (lp[2] - b[2]);
  const double cc = (lp[0] - a[0]) * (lp[1] - b[1]) - (lp[1] - a[1]) * (lp[0] - b[0]);
  const double m = sqrt(ca * ca + cb * cb + cc * cc);
  *res = m / k;
  const double dm_dx = (cb * (b[2] - a[2]) + cc * (a[1] - b[1])) / m;
  const double dm_dy = (ca * (a[2] - b[2]) - cc * (a[0] - b[0])) / m;
  const double dm_dz = (-ca * (a[1] - b[1]) + cb * (a[0] - b[0])) / m;
  if (type == BLK_CORNER) {
    J[0] = dm_dx / k; J[1] = dm_dy / k; J[2] = 0.; J[3] = 0.; J[4] = 0.;
    J[5] = (dm_dx * dx_dy + dm_dy * dy_dy + dm_dz * dz_dy) / k;
  } else {
    J[0] = dm_dx / k; J[1] = dm_dy / k; J[2] = dm_dz / k;
    J[3] = (dm_dx * dx_dr + dm_dy * dy_dr + dm_dz * dz_dr) / k;
    J[4] = (dm_dx * dx_dp + dm_dy * dy_dp + dm_dz * dz_dp) / k;
    J[5] = (dm_dx * dx_dy + dm_dy * dy_dy + dm_dz * dz_dy) / k;
  }
}

// ResidualBlock::Evaluate with HuberLoss(a) + Corrector (rho'' <= 0): accumulates the
// upper triangle of J^T J (21), J^T r (6) and the cost (1) into acc[28].
SOLVE_FN void accumulate_block(double r, const double J[6], double huber_a, double acc[28]) {
  const double s = r * r, b2 = huber_a * huber_a;
  double rho0, rho1;
  if (s > b2) { const double rr = sqrt(s); rho0 = 2.0 * huber_a * rr - b2; rho1 = fmax(2.2250738585072014e-308, huber_a / rr); }
  else { rho0 = s; rho1 = 1.0; }
  const double sq = s > b2 ? sqrt(rho1) : 1.0;  // inliers: rho' = 1, no correction
  double Jc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) Jc[k] = J[k] * sq;
  const double rc = r * sq;
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[t++] += Jc[i] * Jc[j];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[21 + k] += Jc[k] * rc;
  acc[27] += 0.5 * rho0;
}

// accumulate_block for a block type whose Jacobian is a hard zero outside the columns of COLS (bit k = column k): LaserOdometry's surf rows
// (column 2) and corner rows (columns 0, 1, 5).  The terms left out are products with a +0.0 factor; for finite factors they are +-0.0, and adding
// +-0.0 changes no accumulator (one that starts at +0.0 never becomes -0.0).  A row whose residual, corrector or Jacobian is not finite would
// put NaNs into the skipped entries: it takes the generic sums, chosen by one test.  All 28 scalars are the bits accumulate_block delivers.
template <int COLS>
SOLVE_FN void accumulate_block_cols(double r, const double J[6], double huber_a, double acc[28]) {
  const double s = r * r, b2 = huber_a * huber_a;
  double rho0, rho1;
  if (s > b2) { const double rr = sqrt(s); rho0 = 2.0 * huber_a * rr - b2; rho1 = fmax(2.2250738585072014e-308, huber_a / rr); }
  else { rho0 = s; rho1 = 1.0; }
  const double sq = s > b2 ? sqrt(rho1) : 1.0;
  bool fin = isfinite(r) && isfinite(sq);
#pragma unroll
  for (int k = 0; k < 6; ++k) if ((COLS >> k) & 1) fin = fin && isfinite(J[k]);
  double Jc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) Jc[k] = J[k] * sq;
  const double rc = r * sq;
  if (fin) {
    int t = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++t) if (((COLS >> i) & 1) && ((COLS >> j) & 1)) acc[t] += Jc[i] * Jc[j];
#pragma unroll
    for (int k = 0; k < 6; ++k) if ((COLS >> k) & 1) acc[21 + k] += Jc[k] * rc;
  } else {
    int t = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) acc[t++] += Jc[i] * Jc[j];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[21 + k] += Jc[k] * rc;
  }
  acc[27] += 0.5 * rho0;
}
enum { COLS_SURF = 1 << 2, COLS_CORNER = (1 << 0) | (1 << 1) | (1 << 5) };   // the columns eval_block fills for BLK_SURF / BLK_CORNER

// ---- cost-only evaluation: what a trust-region candidate needs (the solvers below evaluate the normal equations only at points a further
// step is computed from).  The residual of a block by exactly the operations eval_block spends on it, the Jacobian left out; accumulate_cost is
// accumulate_block's acc[27] term alone.  Same operations in the same order: the cost of a point is the same double either way.
template <int TYPE>
SOLVE_FN double eval_block_residual(const double cp_[3], const double a[3], const double b[3], const double c[3], double dd, const PoseTerms& T) {
  double lp[3];
  dq_rotate(T.q, cp_, lp);
  lp[0] += T.t[0]; lp[1] += T.t[1]; lp[2] += T.t[2];
  if constexpr (TYPE == BLK_SURF) {
    double ca = (a[1] - b[1]) * (a[2] - c[2]) - (a[2] - b[2]) * (a[1] - c[1]);
    double cb = (a[2] - b[2]) * (a[0] - c[0]) - (a[0] - b[0]) * (a[2] - c[2]);
    double cc = (a[0] - b[0]) * (a[1] - c[1]) - (a[1] - b[1]) * (a[0] - c[0]);
    ca *= ca; cb *= cb; cc *= cc;
    const double ex = lp[0] - a[0], ey = lp[1] - a[1], ez = lp[2] - a[2];
    const double m = sqrt(ex * ex * ca + ey * ey * cb + ez * ez * cc);
    const double k = sqrt(ca + cb + cc);
    return m / k;
  } else if constexpr (TYPE == BLK_PLANE) {
    return (a[0] * lp[0] + a[1] * lp[1] + a[2] * lp[2]) + dd;
  } else {
    const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
    const double k = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    const double ca = (lp[1] - a[1]) * (lp[2] - b[2]) - (lp[2] - a[2]) * (lp[1] - b[1]);
    const double cb = (lp[2] - a[2]) * (lp[0] - b[0]) - (lp[0] - a[0]) * (lp[2] - b[2]);
    const double cc = (lp[0] - a[0]) * (lp[1] - b[1]) - (lp[1] - a[1]) * (lp[0] - b[0]);
    const double m = sqrt(ca * ca + cb * cb + cc * cc);
    return m / k;
  }
}
SOLVE_FN void accumulate_cost(double r, double huber_a, double& cost) {
  const double s = r * r, b2 = huber_a * huber_a;
  double rho0;
  if (s > b2) { const double rr = sqrt(s); rho0 = 2.0 * huber_a * rr - b2; }
  else rho0 = s;
  cost += 0.5 * rho0;
}

// ---------------------------------------------------------------------------
// Trust-region Levenberg-Marquardt control (Ceres TrustRegionMinimizer +
// LevenbergMarquardtStrategy defaults) driven by one thread; the
// residual evaluations are done by the whole workgroup between its steps.
// The DENSE_QR solve of [J; D] y = [r; 0] is replaced by the equivalent normal
// equations (J^T J + D^2) y = J^T r with a 6x6 Cholesky factorisation.
// ---------------------------------------------------------------------------
struct LmState {
  double x[6], cand[6], scale[6], x_cost, x_norm, gmax, radius, dec, mcc;
  double H[21], g[6];   // unscaled J^T J (upper) and J^T r at x
  int iter, max_iter, num_invalid, step_successful, successful, termination;
  int jac_valid;        // H, g and gmax belong to x (a point adopted from a cost-only evaluation clears it)
  double initial_cost;
};
// LM_JAC / LM_EVAL_FULL: only lm_propose_lazy returns them (the normal equations at x are missing / the candidate is evaluated in full)
enum { LM_STOP = 0, LM_EVAL = 1, LM_AGAIN = 2, LM_JAC = 3, LM_EVAL_FULL = 4 };
// what a solver workgroup evaluates next, and what its control thread does with the sums (lm_control)
enum { LM_EV_BEGIN = 0, LM_EV_AGAIN, LM_EV_JAC, LM_EV_CAND_FULL, LM_EV_CAND_COST };

SOLVE_FN int tri(int i, int j) { return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j); }

SOLVE_FN void lm_load_eval(LmState& S, const double* acc) {
#pragma unroll
  for (int k = 0; k < 21; ++k) S.H[k] = acc[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) S.g[k] = acc[21 + k];
  double gm = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gm = fmax(gm, fabs(S.x[k] - (S.x[k] - S.g[k])));
  S.gmax = gm;
  S.jac_valid = 1;
}

SOLVE_FN void lm_begin(LmState& S, const double* x0, const double* acc, int max_iter) {
  double xn = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) { S.x[k] = x0[k]; xn += x0[k] * x0[k]; }
  S.x_norm = sqrt(xn);
  S.x_cost = acc[27]; S.initial_cost = acc[27];
  lm_load_eval(S, acc);
#pragma unroll
  for (int k = 0; k < 6; ++k) S.scale[k] = 1.0 / (1.0 + sqrt(S.H[tri(k, k)]));  // jacobi scaling, iteration 0 only
  S.radius = 1e4; S.dec = 2.0; S.iter = 0; S.max_iter = max_iter; S.num_invalid = 0;
  S.step_successful = 1; S.successful = 0; S.termination = 0;
  if (!isfinite(S.x_cost)) S.termination = 4;
}

// the next candidate into S.cand from the normal equations at S.x (the part of lm_propose behind its stopping tests)
// REMAP (lm_solve_remap; remap_math.h) with proj != null: the step is replaced by S^-1 P S step, P = proj[36] in parameter
// space, before the model cost change is formed — mcc, the candidate and both tests of lm_consume_eval see the projected step.  A projected step
// that is exactly zero (P = 0: every direction is held) is not an invalid step: the candidate is x itself, and its evaluation ends the solve by
// the step-size test (termination 2).  proj == null, or REMAP false: the code below is lm_step as it always was.
template <bool REMAP = false>
SOLVE_FN int lm_step(LmState& S, const double* proj = nullptr) {
  ++S.iter;
  double A[6][6], gs[6], y[6], Hl[21], sc[6], gl[6];
#pragma unroll
  for (int k = 0; k < 21; ++k) Hl[k] = S.H[k];  // LDS -> registers once
#pragma unroll
  for (int k = 0; k < 6; ++k) { sc[k] = S.scale[k]; gl[k] = S.g[k]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    gs[i] = gl[i] * sc[i];
#pragma unroll
    for (int j = 0; j < 6; ++j) A[i][j] = Hl[tri(i, j)] * sc[i] * sc[j];
  }
  double Hs[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) Hs[i][j] = A[i][j];
#pragma unroll
  for (int i = 0; i < 6; ++i) A[i][i] += fmin(fmax(Hs[i][i], 1e-6), 1e32) / S.radius;
  // Cholesky A = L L^T; the diagonal is stored inverted: one division per column instead of one per entry (this thread
  // is the serial part of every solver iteration, and an fp64 division is ~30 instructions)
  bool ok = true;
  double dinv[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int k = 0; k < j; ++k) s -= A[j][k] * A[j][k];
    if (!(s > 0)) { ok = false; s = 1; }
    const double l = sqrt(s);
    dinv[j] = 1.0 / l;
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
      for (int k = 0; k < j; ++k) t -= A[i][k] * A[j][k];
      A[i][j] = t * dinv[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) { double t = gs[i]; for (int k = 0; k < i; ++k) t -= A[i][k] * y[k]; y[i] = t * dinv[i]; }
#pragma unroll
  for (int i = 5; i >= 0; --i) { double t = y[i]; for (int k = i + 1; k < 6; ++k) t -= A[k][i] * y[k]; y[i] = t * dinv[i]; }
  double step[6], mcc = 0;
  bool finite = ok;
#pragma unroll
  for (int i = 0; i < 6; ++i) { step[i] = -y[i]; finite = finite && isfinite(step[i]); }
  bool null_step = false;
  if constexpr (REMAP) {
    if (proj && finite) {
      SOLVE_SCHED_FENCE();   // (the 36 loads of P stay behind the factorisation: hoisted above it they cost the kernel a wavefront per SIMD)
      rm_project_step(proj, sc, step);
      SOLVE_SCHED_FENCE();
      null_step = true;
#pragma unroll
      for (int i = 0; i < 6; ++i) { finite = finite && isfinite(step[i]); null_step = null_step && step[i] == 0.0; }
    }
  }
  if (finite) {
    double lin = 0, quad = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      lin += step[i] * gs[i];
      double t = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) t += Hs[i][j] * step[j];
      quad += step[i] * t;
    }
    mcc = -lin - 0.5 * quad;
  }
  if constexpr (REMAP) {
    if (finite && null_step) {   // (mcc is 0: lm_consume_eval's step-size test ends the solve before it is read)
      S.num_invalid = 0;
      S.mcc = mcc;
#pragma unroll
      for (int i = 0; i < 6; ++i) S.cand[i] = S.x[i] + step[i] * sc[i];
      return LM_EVAL;
    }
  }
  if (!finite || !(mcc > 0.0)) {  // HandleInvalidStep
    if (++S.num_invalid >= 5) { S.termination = 4; return LM_STOP; }
    S.radius /= S.dec; S.dec *= 2.0; S.step_successful = 0;
    return LM_AGAIN;
  }
  S.num_invalid = 0;
  S.mcc = mcc;
#pragma unroll
  for (int i = 0; i < 6; ++i) S.cand[i] = S.x[i] + step[i] * sc[i];
  return LM_EVAL;
}

// decide whether to stop, and if not compute the next candidate into S.cand
template <bool REMAP = false>
SOLVE_FN int lm_propose(LmState& S, const double* proj = nullptr) {
  if (S.termination == 4) return LM_STOP;
  if (S.iter >= S.max_iter) { S.termination = 0; return LM_STOP; }
  if (S.step_successful && S.gmax <= 1e-10) { S.termination = 1; return LM_STOP; }
  if (S.radius <= 1e-32) { S.termination = 5; return LM_STOP; }
  return lm_step<REMAP>(S, proj);
}

// lm_propose for a solver that evaluates candidates for their cost alone.  The stopping tests that read neither H nor g come first; LM_JAC asks
// the caller for the normal equations at S.x (lm_load_eval) and another call; the remaining tests then run in lm_propose's order.  (jac_valid is
// cleared only by a successful step, so after an unsuccessful one the radius test below is reached without an evaluation.)
// SPECULATE: the candidate after a successful step is evaluated in full (LM_EVAL_FULL), so that adopting it costs no second pass.
template <bool SPECULATE, bool REMAP = false>
SOLVE_FN int lm_propose_lazy(LmState& S, const double* proj = nullptr) {
  if (S.termination == 4) return LM_STOP;
  if (S.iter >= S.max_iter) { S.termination = 0; return LM_STOP; }
  if (!S.jac_valid) return LM_JAC;
  if (S.step_successful && S.gmax <= 1e-10) { S.termination = 1; return LM_STOP; }
  if (S.radius <= 1e-32) { S.termination = 5; return LM_STOP; }
  const int prev_successful = S.step_successful;
  const int act = lm_step<REMAP>(S, proj);
  return (SPECULATE && act == LM_EVAL && prev_successful) ? LM_EVAL_FULL : act;
}

// a further ceres::Solve from the point the last one ended at, when the normal equations there are still held (S.jac_valid): what lm_begin
// would take from a fresh evaluation at S.x is what S holds — the evaluation is a function of x and the rows, and neither has changed
SOLVE_FN void lm_begin_again(LmState& S, int max_iter) {
  S.initial_cost = S.x_cost;
#pragma unroll
  for (int k = 0; k < 6; ++k) S.scale[k] = 1.0 / (1.0 + sqrt(S.H[tri(k, k)]));
  S.radius = 1e4; S.dec = 2.0; S.iter = 0; S.max_iter = max_iter; S.num_invalid = 0;
  S.step_successful = 1; S.successful = 0; S.termination = 0;
  if (!isfinite(S.x_cost)) S.termination = 4;
}

// consume the evaluation at S.cand; returns LM_STOP on convergence.  full: acc holds the normal equations at S.cand; otherwise only acc[27]
SOLVE_FN int lm_consume_eval(LmState& S, const double* acc, bool full) {
  double cand_cost = acc[27];
  if (!isfinite(cand_cost)) cand_cost = 1.7976931348623157e308;
  double sn = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) sn += (S.x[k] - S.cand[k]) * (S.x[k] - S.cand[k]);
  if (sqrt(sn) <= 1e-8 * (S.x_norm + 1e-8)) { S.termination = 2; return LM_STOP; }
  const double cost_change = S.x_cost - cand_cost;
  if (fabs(cost_change) <= 1e-6 * S.x_cost) { S.termination = 3; return LM_STOP; }
  const double rd = cost_change / S.mcc;
  if (rd > 1e-3) {
    double xn = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { S.x[k] = S.cand[k]; xn += S.x[k] * S.x[k]; }
    S.x_norm = sqrt(xn);
    S.x_cost = cand_cost;
    if (full) lm_load_eval(S, acc); else S.jac_valid = 0;
    S.step_successful = 1; ++S.successful;
    const double t = 2.0 * rd - 1.0;
    S.radius = S.radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
    S.radius = fmin(1e16, S.radius);
    S.dec = 2.0;
  } else {
    S.step_successful = 0;
    S.radius /= S.dec; S.dec *= 2.0;
  }
  return LM_AGAIN;
}
// One turn of the control thread of lo_solve_t / lm_solve: take in the evaluation of `kind`, then propose until there is something to evaluate or
// the solve has ended.  x0: the point of LM_EV_BEGIN.  FULL_EVAL: lm_propose, every candidate in full — call for call the solver before the split.
// REMAP, proj: lm_step's.
template <bool FULL_EVAL, bool SPECULATE, bool REMAP = false>
SOLVE_FN int lm_control(LmState& S, int kind, const double* x0, const double* sums, int max_iter, const double* proj = nullptr) {
  int act = LM_AGAIN;
  if (kind == LM_EV_BEGIN) lm_begin(S, x0, sums, max_iter);
  else if (kind == LM_EV_AGAIN) lm_begin_again(S, max_iter);
  else if (kind == LM_EV_JAC) lm_load_eval(S, sums);
  else act = lm_consume_eval(S, sums, kind == LM_EV_CAND_FULL);
  while (act == LM_AGAIN) act = FULL_EVAL ? lm_propose<REMAP>(S, proj) : lm_propose_lazy<SPECULATE, REMAP>(S, proj);
  return act;
}
// ... and the evaluation that answer asks for
template <bool FULL_EVAL>
SOLVE_FN int lm_next_eval(int act) { return (!FULL_EVAL && act == LM_JAC) ? LM_EV_JAC : (FULL_EVAL || act == LM_EVAL_FULL) ? LM_EV_CAND_FULL : LM_EV_CAND_COST; }
SOLVE_FN int lm_consume(LmState& S, const double* acc) { return lm_consume_eval(S, acc, true); }

#endif
