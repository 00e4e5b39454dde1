// align_math.h — the rule of alego_map_align that decides between the answers of several queries, shared by the
// kernel (ma_consensus, kernels_reloc.hip) and the host twins (alego_map_align_queries / alego_map_align_consensus): one definition, so the
// two cannot drift apart.  Plain C++ that a host compiler reads without the HIP runtime; f64 without contraction (-ffp-contract=off).
//
// QUERIES: Q = min(n_queries, ns) of the ns archived source frames; query q is frame ((2 q + 1) ns) / (2 Q) in integer arithmetic, the
// middle of the q-th of Q equal stretches: distinct and ascending, since consecutive values differ by ns / Q >= 1 before the floor.
// HYPOTHESIS: a row-major 4 x 4 f32 T (dst <- src; rows 0 .. 2 are read) and the f32 position p of the query's source key pose.
// AGREE(a, b): with M = R_a^T R_b (f32 widened to f64, every sum left to right), c = (tr M - 1) / 2, v = vee(M - M^T) / 2, the angle
// atan2(|v|, c) (as pg_math.h's Logmap takes it) must be <= tol_rot, and at p = p_a and at p = p_b the distance
// |(R_a p + t_a) - (R_b p + t_b)| must be <= tol_trans.  Positions are compared rather than the translation columns, so that a small
// rotation error far from the origin counts.  Every comparison is written so that a NaN fails it: a non-finite T agrees with nothing, itself
// included.  AGREE(a, b) == AGREE(b, a) bit for bit: M becomes its transpose, v its negative and each difference its negative.
// SUPPORT(a) = the accepted b with AGREE(a, b), a itself among them (0 for a hypothesis that is not accepted or not finite).
// BEST = the accepted hypothesis with support >= 1 that is largest in support, then smallest in fitness (ma_fit_key: the order of `<` on
// doubles as an order of u64), then smallest in index; -1 when there is none.  No averaging: the result is the best hypothesis itself.
#ifndef ALEGO_ALIGN_MATH_H_
#define ALEGO_ALIGN_MATH_H_
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define MA_FN __host__ __device__ inline
#else
#define MA_FN inline
#endif

#define MA_MAX_QUERIES 32   // ALEGO_ALIGN_MAX_QUERIES: one lane per hypothesis leaves half a wavefront idle and keeps a row of the tables small

MA_FN int ma_query_count(int ns, int n_queries) { return ns < n_queries ? (ns > 0 ? ns : 0) : n_queries; }
MA_FN int ma_query_frame(int ns, int Q, int q) { return (int)(((long long)(2 * q + 1) * (long long)ns) / (long long)(2 * Q)); }

MA_FN bool ma_agree(const float* Ta, const float* pa, const float* Tb, const float* pb, double tol_trans, double tol_rot) {
  double M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      M[i * 3 + j] = ((double)Ta[0 + i] * (double)Tb[0 + j] + (double)Ta[4 + i] * (double)Tb[4 + j]) + (double)Ta[8 + i] * (double)Tb[8 + j];
  const double c = 0.5 * (((M[0] + M[4]) + M[8]) - 1.0);
  const double v[3] = {0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1])};
  const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  if (!(atan2(s, c) <= tol_rot)) return false;
  for (int k = 0; k < 2; ++k) {
    const float* p = k ? pb : pa;
    double d[3];
    for (int r = 0; r < 3; ++r) {
      const double ya = (((double)Ta[r * 4 + 0] * (double)p[0] + (double)Ta[r * 4 + 1] * (double)p[1]) + (double)Ta[r * 4 + 2] * (double)p[2]) + (double)Ta[r * 4 + 3];
      const double yb = (((double)Tb[r * 4 + 0] * (double)p[0] + (double)Tb[r * 4 + 1] * (double)p[1]) + (double)Tb[r * 4 + 2] * (double)p[2]) + (double)Tb[r * 4 + 3];
      d[r] = ya - yb;
    }
    if (!(sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= tol_trans)) return false;
  }
  return true;
}

// a u64 whose order by `<` is the order of the doubles by `<` (-0.0 below +0.0; NaNs at the two ends, by their sign)
MA_FN unsigned long long ma_fit_key(double f) {
  unsigned long long b;
  __builtin_memcpy(&b, &f, sizeof(b));
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// support[a] of hypotheses 0 .. n - 1 (T16[n][16], p3[n][3]) and the best one; returns its index or -1
MA_FN int ma_consensus_ref(const float* T16, const float* p3, const double* fitness, const int32_t* accepted, int n, double tol_trans, double tol_rot, int32_t* support) {
  int best = -1;
  for (int a = 0; a < n; ++a) {
    int s = 0;
    for (int b = 0; b < n; ++b)
      if (accepted[a] && accepted[b] && ma_agree(T16 + (size_t)a * 16, p3 + (size_t)a * 3, T16 + (size_t)b * 16, p3 + (size_t)b * 3, tol_trans, tol_rot)) ++s;
    support[a] = s;
    if (s < 1) continue;
    if (best < 0 || s > support[best] || (s == support[best] && ma_fit_key(fitness[a]) < ma_fit_key(fitness[best]))) best = a;
  }
  return best;
}

#endif
