// remap_math.h — solution remapping of LaserMapping's scan-to-map registration (Zhang, Kaess, Singh, "On degeneracy of
// optimization-based state estimation problems", ICRA 2016; LOAM / LeGO-LOAM's matP), f64 throughout, shared by the solver kernels
// (lm_solve_remap, kernels_lm.hip) and the host twins (alego_remap_host, alego_remap_step_host); readable by a host compiler without the HIP
// runtime, as reg_cov_math.h is (tests/remap_math/remap_math_check.cpp compiles the two headers and solve_rows.h alone).
//
// Input: the 28 scalars of the solver's first evaluation of a mapping frame, at the point x0 its first outer solve starts from.
//   where     the tangent space of reg_cov_math.h: info = N^T H N, N = M(x0)^-1 (rc_minv, rc_info_entry), the cyclic Jacobi of that header
//             (rc_jacobi on the host, the same rotations entry by entry on 36 lanes in the kernel), ascending, ties by index (rc_rank)
//   held      eigval[k] < eig_min: a direction alego_regcov would count as degenerate at x0
//   Pt        sum over the kept k of v_k v_k^T, entry (i, j) as the sum of (V_ik V_jk) in ascending k: symmetric to the last bit
//   P         N Pt M, 6x6 row-major, in parameter space: entry (i, j) = sum_a N_ia (sum_b Pt_ab M_bj), both sums ascending from 0.0
//   step      lm_step (solve_rows.h) replaces its step by S^-1 P S step, S = diag(scale): t_j = scale_j step_j, u_i = sum_j P_ij t_j ascending
//             from 0.0, step_i = u_i / scale_i (rm_project_step), before the model cost change is formed
// n_held == 0: P is the exact identity and the solver is told nothing is held (its step is not touched); n_held == 6: P is exactly zero.
// Status: 1 computed; 0 fewer than 7 rows; -3 |cos pitch| < RC_COS_PITCH_MIN; -2 an input or a result is not finite.  With a status other than 1
// nothing is held and every double of the result is zero.  The first three guards, their order and the tie rule are rc_spectrum's (reg_cov_math.h),
// the front alego_regcov shares: n_held here and n_degenerate there cannot disagree at equal eig_min.
#ifndef ALEGO_REMAP_MATH_H_
#define ALEGO_REMAP_MATH_H_
#include "reg_cov_math.h"

// the option: NULL or <= 0 = RC_DEFAULT_EIG_MIN; -1: not finite
RC_FN int rm_resolve(const double* raw_eig_min, double* eig_min) {
  *eig_min = RC_DEFAULT_EIG_MIN;
  if (raw_eig_min) {
    if (!rc_finite(*raw_eig_min)) return -1;
    if (*raw_eig_min > 0.0) *eig_min = *raw_eig_min;
  }
  return 0;
}
RC_FN bool rm_kept(double lam, double eig_min) { return !(lam < eig_min); }
// Pt(i, j) from rows i and j of the sorted eigenvectors
RC_FN double rm_pt_entry(const double* vi, const double* vj, const double* lam, double eig_min) {
  double s = 0.0;
RC_UNROLL
  for (int k = 0; k < 6; ++k) s += rm_kept(lam[k], eig_min) ? vi[k] * vj[k] : 0.0;
  return s;
}
// (Pt M)(a, j) from row a of Pt and M
RC_FN double rm_ptm_entry(const double* pt_row, const double* M, int j) {
  double t = 0.0;
RC_UNROLL
  for (int b = 0; b < 6; ++b) t += pt_row[b] * M[b * 6 + j];
  return t;
}
// P(i, j) from column j of Pt M and N
RC_FN double rm_p_entry(const double* N, int i, const double* ptm_col) {
  double s = 0.0;
RC_UNROLL
  for (int a = 0; a < 6; ++a) s += N[i * 6 + a] * ptm_col[a];
  return s;
}
// step <- S^-1 P S step
RC_FN void rm_project_step(const double* P, const double* scale, double* step) {
  double t[6], u[6];
RC_UNROLL
  for (int j = 0; j < 6; ++j) t[j] = scale[j] * step[j];
RC_UNROLL
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
RC_UNROLL
    for (int j = 0; j < 6; ++j) s += P[i * 6 + j] * t[j];
    u[i] = s;
  }
RC_UNROLL
  for (int i = 0; i < 6; ++i) step[i] = u[i] / scale[i];
}

// The decomposition as plain arrays (the host twin; the kernel does the same entry by entry on 36 lanes): the projector tail of rc_spectrum
// (reg_cov_math.h), which owns the guards.  Returns the status.
RC_FN int rm_compute(const double* acc, const double* p, int n_edge, int n_plane, double eig_min, double* eigval, double* eigvec, double* proj, int* n_held) {
  *n_held = 0;
  for (int k = 0; k < 36; ++k) { eigvec[k] = 0.0; proj[k] = 0.0; }
  for (int k = 0; k < 6; ++k) eigval[k] = 0.0;
  double N[36], M[36], info[36], lam[6], Vs[36], Pt[36], PtM[36], P[36];
  const int st = rc_spectrum(acc, p, n_edge, n_plane, N, info, lam, Vs, nullptr);
  if (st != 1) return st;
  rc_m(p, M);
  int held = 0;
  for (int k = 0; k < 6; ++k) held += rm_kept(lam[k], eig_min) ? 0 : 1;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) Pt[i * 6 + j] = rm_pt_entry(Vs + i * 6, Vs + j * 6, lam, eig_min);
  for (int a = 0; a < 6; ++a)
    for (int j = 0; j < 6; ++j) PtM[a * 6 + j] = rm_ptm_entry(Pt + a * 6, M, j);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double col[6];
      for (int a = 0; a < 6; ++a) col[a] = PtM[a * 6 + j];
      const double v = rm_p_entry(N, i, col);
      P[i * 6 + j] = held == 0 ? (i == j ? 1.0 : 0.0) : (held == 6 ? 0.0 : v);
    }
  bool bad = false;
  for (int k = 0; k < 36; ++k) bad = bad || !rc_finite(Vs[k]) || !rc_finite(P[k]);
  for (int k = 0; k < 6; ++k) bad = bad || !rc_finite(lam[k]);
  if (bad) return -2;
  *n_held = held;
  for (int k = 0; k < 36; ++k) { eigvec[k] = Vs[k]; proj[k] = P[k]; }
  for (int k = 0; k < 6; ++k) eigval[k] = lam[k];
  return 1;
}

#endif
