// pg_math.h — the arithmetic of the key-pose graph, f64 throughout, shared by the device kernels
// (kernels_graph.hip) and the host-only entry point alego_graph_residuals: Pose3 as a row-major 3x4 [R | t], the full SE(3)
// Logmap / Expmap in GTSAM's tangent order (rotation first), and the whitened error of a Between / prior factor with its two 6x6
// Jacobian blocks for the update x <- x Expmap(delta), in closed form.
#ifndef ALEGO_PG_MATH_H_
#define ALEGO_PG_MATH_H_
#include <math.h>

#if defined(__HIPCC__)
#define PG_FN __host__ __device__ inline
#else
#define PG_FN inline
#endif

// below this angle the coefficients that cancel (pg_coef_c, pg_coef_dc, pg_coef_v) come from their series
#define PG_SERIES_THETA 0.1

// Rot3::RzRyRx(roll, pitch, yaw)
PG_FN void pg_rzryrx(double roll, double pitch, double yaw, double* R) {
  const double cx = cos(roll), sx = sin(roll), cy = cos(pitch), sy = sin(pitch), cz = cos(yaw), sz = sin(yaw);
  const double ss_ = sx * sy, cs_ = cx * sy, sc_ = sx * cy, cc_ = cx * cy, c_s = cx * sz, s_s = sx * sz, _cs = cy * sz, _cc = cy * cz, s_c = sx * cz, c_c = cx * cz;
  const double ssc = ss_ * cz, csc = cs_ * cz, sss = ss_ * sz, css = cs_ * sz;
  R[0] = _cc; R[1] = -c_s + ssc; R[2] = s_s + csc; R[3] = _cs; R[4] = c_c + sss; R[5] = -s_c + css; R[6] = -sy; R[7] = sc_; R[8] = cc_;
}
// Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)) of an f32 key pose (x y z roll pitch yaw)
PG_FN void pg_from_pose6(const float* kp, double* X) {
  double R[9];
  pg_rzryrx((double)kp[3], (double)kp[4], (double)kp[5], R);
  for (int r = 0; r < 3; ++r) { X[r * 4 + 0] = R[r * 3 + 0]; X[r * 4 + 1] = R[r * 3 + 1]; X[r * 4 + 2] = R[r * 3 + 2]; X[r * 4 + 3] = (double)kp[r]; }
}
// the f32 key pose of a Pose3: x y z, then gtsam::Rot3::roll / pitch / yaw (the formulas of lm_finish, laserMapping.cpp:572-577)
PG_FN void pg_to_pose6(const double* X, float* kp) {
  kp[0] = (float)X[3]; kp[1] = (float)X[7]; kp[2] = (float)X[11];
  kp[3] = (float)atan2(X[9], X[10]);
  kp[4] = (float)atan2(-X[8], sqrt(X[9] * X[9] + X[10] * X[10]));
  kp[5] = (float)atan2(X[4], X[0]);
}
// Pose3::between: A^-1 B
PG_FN void pg_between(const double* A, const double* B, double* O) {
  const double d[3] = {B[3] - A[3], B[7] - A[7], B[11] - A[11]};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) O[r * 4 + c] = (A[0 + r] * B[0 + c] + A[4 + r] * B[4 + c]) + A[8 + r] * B[8 + c];
    O[r * 4 + 3] = (A[0 + r] * d[0] + A[4 + r] * d[1]) + A[8 + r] * d[2];
  }
}
// Pose3::compose: A B
PG_FN void pg_compose(const double* A, const double* B, double* O) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) O[r * 4 + c] = (A[r * 4 + 0] * B[0 + c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c];
    O[r * 4 + 3] += A[r * 4 + 3];
  }
}

// c(theta) = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta): the W^2 coefficient of the SO(3) Jacobian inverses
PG_FN double pg_coef_c(double th) {
  if (th < PG_SERIES_THETA) { const double t2 = th * th; return 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 * (1.0 / 47900160)))); }
  const double h = 0.5 * th;
  return (1.0 - h * cos(h) / sin(h)) / (th * th);
}
// c'(theta) / theta
PG_FN double pg_coef_dc(double th) {
  if (th < PG_SERIES_THETA) { const double t2 = th * th; return 1.0 / 360 + t2 * (1.0 / 7560 + t2 * (1.0 / 201600 + t2 * (1.0 / 5987520))); }
  const double h = 0.5 * th, sh = sin(h), ct = cos(h) / sh, t2 = th * th;
  return (-2.0 / (t2 * th) + 1.0 / (4.0 * th * sh * sh) + ct / (2.0 * t2)) / th;
}
// (theta - sin theta) / theta^3: the W^2 coefficient of Expmap's V
PG_FN double pg_coef_v(double th) {
  if (th < PG_SERIES_THETA) { const double t2 = th * th; return 1.0 / 6 - t2 * (1.0 / 120 - t2 * (1.0 / 5040 - t2 * (1.0 / 362880 - t2 * (1.0 / 39916800)))); }
  return (th - sin(th)) / (th * th * th);
}

PG_FN void pg_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// Pose3::Logmap, full SE(3): xi = (omega, u) with R = Exp(omega), t = V(omega) u.  The angle comes from atan2(|v|, c) with
// v = vee(R - R^T) / 2, c = (tr R - 1) / 2; the axis from v, or beyond 120 degrees from the symmetric part of R, where v vanishes.
PG_FN void pg_log(const double* T, double* xi) {
  const double c = 0.5 * ((T[0] + T[5] + T[10]) - 1.0);
  const double v[3] = {0.5 * (T[9] - T[6]), 0.5 * (T[2] - T[8]), 0.5 * (T[4] - T[1])};
  const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double th = atan2(s, c);
  double w[3];
  if (c > -0.5) {
    const double f = s > 1e-10 ? th / s : 1.0;
    w[0] = f * v[0]; w[1] = f * v[1]; w[2] = f * v[2];
  } else {
    // (R + R^T) / 2 - c I = (1 - c) a a^T: the column of the largest diagonal entry, signed by v
    const double d[3] = {T[0] - c, T[5] - c, T[10] - c};
    const int k = d[0] >= d[1] ? (d[0] >= d[2] ? 0 : 2) : (d[1] >= d[2] ? 1 : 2);
    double a[3];
    for (int i = 0; i < 3; ++i) a[i] = i == k ? d[k] : 0.5 * (T[i * 4 + k] + T[k * 4 + i]);
    double f = th / sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if ((a[0] * v[0] + a[1] * v[1]) + a[2] * v[2] < 0.0) f = -f;
    w[0] = f * a[0]; w[1] = f * a[1]; w[2] = f * a[2];
  }
  const double t[3] = {T[3], T[7], T[11]};
  double wt[3], wwt[3];
  pg_cross(w, t, wt);
  pg_cross(w, wt, wwt);
  const double cc = pg_coef_c(th);
  for (int i = 0; i < 3; ++i) { xi[i] = w[i]; xi[3 + i] = (t[i] - 0.5 * wt[i]) + cc * wwt[i]; }
}

// Pose3::Expmap, full SE(3)
PG_FN void pg_exp(const double* xi, double* T) {
  const double w[3] = {xi[0], xi[1], xi[2]};
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(t2);
  double a = 1.0, b = 0.5;
  if (th > 1e-10) { const double sh = sin(0.5 * th) / (0.5 * th); a = sin(th) / th; b = 0.5 * sh * sh; }
  const double cv = pg_coef_v(th);
  const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double W2[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) W2[r * 3 + c] = w[r] * w[c] - (r == c ? t2 : 0.0);
  for (int r = 0; r < 3; ++r) {
    double tr = 0.0;
    for (int c = 0; c < 3; ++c) {
      const double I = r == c ? 1.0 : 0.0;
      T[r * 4 + c] = (I + a * W[r * 3 + c]) + b * W2[r * 3 + c];
      tr += ((I + b * W[r * 3 + c]) + cv * W2[r * 3 + c]) * xi[3 + c];
    }
    T[r * 4 + 3] = tr;
  }
}

// xi = Logmap(T) and J = d Logmap(T Expmap(d)) / d d at d = 0 (Pose3::LogmapDerivative; row-major 6x6):
//   [ Jr^-1(omega)        0        ]      Jr^-1(omega) = I + W / 2 + c W^2
//   [ D Jr^-1(omega)   Jr^-1(omega) ]      D = d (Jl^-1(omega) t) / d omega at fixed t
//                                           = [t]x / 2 + c ((omega . t) I + omega t^T - 2 t omega^T) + (c' / theta) (W^2 t) omega^T
PG_FN void pg_log_jac(const double* T, double* xi, double* J) {
  pg_log(T, xi);
  const double w[3] = {xi[0], xi[1], xi[2]}, t[3] = {T[3], T[7], T[11]};
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(t2);
  const double cc = pg_coef_c(th), dc = pg_coef_dc(th);
  const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  const double Tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  double Ji[9], D[9], wt[3], wwt[3];
  pg_cross(w, t, wt);
  pg_cross(w, wt, wwt);
  const double wdt = (w[0] * t[0] + w[1] * t[1]) + w[2] * t[2];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double I = r == c ? 1.0 : 0.0;
      Ji[r * 3 + c] = (I + 0.5 * W[r * 3 + c]) + cc * (w[r] * w[c] - I * t2);
      D[r * 3 + c] = (0.5 * Tx[r * 3 + c] + cc * ((wdt * I + w[r] * t[c]) - 2.0 * t[r] * w[c])) + dc * wwt[r] * w[c];
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      J[r * 6 + c] = Ji[r * 3 + c];
      J[r * 6 + 3 + c] = 0.0;
      J[(3 + r) * 6 + c] = (D[r * 3 + 0] * Ji[0 + c] + D[r * 3 + 1] * Ji[3 + c]) + D[r * 3 + 2] * Ji[6 + c];
      J[(3 + r) * 6 + 3 + c] = Ji[r * 3 + c];
    }
}

// One factor.  xf == nullptr: PriorFactor<Pose3> on xt with the prior `meas`, error Logmap(meas^-1 xt); else BetweenFactor<Pose3>,
// error Logmap(meas^-1 (xf^-1 xt)).  res = the error whitened by 1 / sqrt(var); Jf, Jt = d res / d delta_from, d delta_to for
// x <- x Expmap(delta) (row-major 6x6; Jf = 0 for a prior).
PG_FN void pg_factor(const double* xf, const double* xt, const double* meas, const double* var, double* res, double* Jf, double* Jt) {
  double h[12], e[12], J[36];
  if (xf) {
    pg_between(xf, xt, h);
    pg_between(meas, h, e);
  } else {
    pg_between(meas, xt, e);
  }
  pg_log_jac(e, res, J);
  double sw[6];
  for (int r = 0; r < 6; ++r) { sw[r] = 1.0 / sqrt(var[r]); res[r] *= sw[r]; }
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) Jt[r * 6 + c] = J[r * 6 + c] * sw[r];
  if (!xf) {
    for (int i = 0; i < 36; ++i) Jf[i] = 0.0;
    return;
  }
  // d (xf^-1 xt) / d delta_from = -Ad(h^-1) = -[ R^T 0 ; -R^T [t]x  R^T ]
  double Ad[36];
  const double t[3] = {h[3], h[7], h[11]};
  const double Tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double rt = h[c * 4 + r];
      Ad[r * 6 + c] = -rt; Ad[r * 6 + 3 + c] = 0.0; Ad[(3 + r) * 6 + 3 + c] = -rt;
      Ad[(3 + r) * 6 + c] = (h[0 + r] * Tx[0 + c] + h[4 + r] * Tx[3 + c]) + h[8 + r] * Tx[6 + c];
    }
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double a = 0.0;
      for (int k = 0; k < 6; ++k) a += J[r * 6 + k] * Ad[k * 6 + c];
      Jf[r * 6 + c] = a * sw[r];
    }
}

#endif
