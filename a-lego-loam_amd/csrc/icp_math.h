// icp_math.h — the per-iteration arithmetic of pcl::IterativeClosestPoint as performLoopClosure configures it
// (laserMapping.cpp:670-692), shared by the single-attempt path (kernels_icp.hip) and the batched search (kernels_loop.hip):
// Horn's closed-form rigid transform from the 17 correspondence sums, accumulation of final_transformation_ and
// DefaultConvergenceCriteria.  One thread runs it.  Plain C++ that a host compiler reads without the HIP runtime (tests/icp_math/icp_math_check.cpp
// runs it against an SVD reference); f64 without contraction (-ffp-contract=off) on both sides.
#ifndef ALEGO_ICP_MATH_H_
#define ALEGO_ICP_MATH_H_
#include <float.h>
#include <math.h>
#include "../../include/alego_params.h"

#ifdef __HIPCC__
#define ICP_FN __host__ __device__ inline
#else
#define ICP_FN inline
#endif

struct IcpState {
  float M[16];        // transformation_ of the last iteration (applied to the source by the next icp_corr)
  float Tf[16];       // final_transformation_
  double prev_mse, fitness;
  int iter, done, converged, apply, n_src, n_tgt;
};

// symmetric 4x4 eigen-decomposition, cyclic Jacobi (same algorithm as oracle_icp.h)
ICP_FN void jacobi4(double A[4][4], double V[4][4], double lam[4]) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int p = 0; p < 4; ++p) for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
    if (off < 1e-300) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
        for (int k = 0; k < 4; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
        for (int k = 0; k < 4; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
      }
  }
  for (int i = 0; i < 4; ++i) lam[i] = A[i][i];
}

// T[17]: sum of source xyz (0..2), target xyz (3..5), source_u * target_w (6 + 3 u + w), squared distances (15), count (16)
ICP_FN void icp_update(IcpState* S, const double* T, const alego_params& P) {
  const double n = T[16];
  if (n < 3.0) { S->done = 1; S->converged = 0; return; }   // "Not enough correspondences found"
  const double mse = T[15] / n;
  const double ms[3] = {T[0] / n, T[1] / n, T[2] / n}, mt[3] = {T[3] / n, T[4] / n, T[5] / n};
  double Mc[3][3];
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) Mc[a][b] = T[6 + a * 3 + b] - n * ms[a] * mt[b];
  double Nq[4][4] = {{Mc[0][0] + Mc[1][1] + Mc[2][2], Mc[1][2] - Mc[2][1], Mc[2][0] - Mc[0][2], Mc[0][1] - Mc[1][0]},
                     {Mc[1][2] - Mc[2][1], Mc[0][0] - Mc[1][1] - Mc[2][2], Mc[0][1] + Mc[1][0], Mc[2][0] + Mc[0][2]},
                     {Mc[2][0] - Mc[0][2], Mc[0][1] + Mc[1][0], -Mc[0][0] + Mc[1][1] - Mc[2][2], Mc[1][2] + Mc[2][1]},
                     {Mc[0][1] - Mc[1][0], Mc[2][0] + Mc[0][2], Mc[1][2] + Mc[2][1], -Mc[0][0] - Mc[1][1] + Mc[2][2]}};
  double V[4][4], lam[4];
  jacobi4(Nq, V, lam);
  int best = 0;
  for (int i = 1; i < 4; ++i) if (lam[i] > lam[best]) best = i;
  double q[4] = {V[0][best], V[1][best], V[2][best], V[3][best]};
  if (q[0] < 0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
  const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / nn, x = q[1] / nn, y = q[2] / nn, z = q[3] / nn;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  float M[16];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) M[a * 4 + b] = (float)R[a * 3 + b];
    M[a * 4 + 3] = (float)(mt[a] - (R[a * 3 + 0] * ms[0] + R[a * 3 + 1] * ms[1] + R[a * 3 + 2] * ms[2]));
  }
  M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
  float Nf[16];   // final_transformation_ = transformation_ * final_transformation_ (Matrix4f)
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Nf[r * 4 + c] = M[r * 4 + 0] * S->Tf[0 * 4 + c] + M[r * 4 + 1] * S->Tf[1 * 4 + c] + M[r * 4 + 2] * S->Tf[2 * 4 + c] + M[r * 4 + 3] * S->Tf[3 * 4 + c];
  for (int k = 0; k < 16; ++k) { S->M[k] = M[k]; S->Tf[k] = Nf[k]; }
  S->apply = 1;
  const int it = ++S->iter;
  // DefaultConvergenceCriteria::hasConverged (absolute MSE 1e-12 is PCL's default; IterativeClosestPoint::computeTransformation sets the
  // rotation threshold to 1 - transformation_epsilon_ (PCL 1.8: setRotationThreshold(1.0 - transformation_epsilon_)), i.e. 0.999999 with laserMapping.cpp:673)
  bool conv = false;
  if (it >= P.icp_max_iters) conv = true;
  else {
    const double cos_angle = 0.5 * ((double)M[0] + (double)M[5] + (double)M[10] - 1.0);
    const double tr2 = (double)M[3] * M[3] + (double)M[7] * M[7] + (double)M[11] * M[11];
    if (cos_angle >= 1.0 - P.icp_trans_eps && tr2 <= P.icp_trans_eps) conv = true;
    else if (fabs(mse - S->prev_mse) < 1e-12) conv = true;
    else if (fabs(mse - S->prev_mse) / S->prev_mse < P.icp_fitness_eps) conv = true;
    else S->prev_mse = mse;
  }
  if (conv) { S->done = 1; S->converged = 1; }
}

#endif
