// pg_cov_math.h — the arithmetic of the key-pose graph's marginal covariances and of the loop-edge gate, f64
// throughout, shared by the device kernels (kernels_pgcov.hip) and the host twin (alego_graph_covariance_host, alego_graph_check_host;
// tests/pg_cov_math/pg_cov_math_check.cpp compiles this header alone with a host compiler).
//
// With the whitened Jacobian J of the graph at the archived poses, Lambda = J^T J = T + Jl^T Jl: T block-tridiagonal (prior + chain),
// Jl the 6 * loops rows of the loop edges.  T = L L^T with L block-bidiagonal (L_kk, L_{k+1,k}); Z = T^-1 Jl^T; C = I + Jl Z = Lc Lc^T.
//   Sigma = Lambda^-1 = T^-1 - Z C^-1 Z^T                                       (Woodbury)
//   S_kk = (T^-1)_kk:  S_{N-1,N-1} = L^-T L^-1 of the last block,  S_kk = L_kk^-T L_kk^-1 + G_k^T S_{k+1,k+1} G_k,  G_k = L_{k+1,k} L_kk^-1
//   W_k = Lc^-1 Z_k^T (6 loops x 6):  Sigma_kk = S_kk - W_k^T W_k,  Sigma_ij = (T^-1)_ij - W_i^T W_j
// A candidate i -> j with the unwhitened error e and Jacobian blocks A (d e / d delta_i), B (d e / d delta_j):
//   P = A Sigma_ii A^T + B Sigma_jj B^T + A Sigma_ij B^T + B Sigma_ij^T A^T + diag(variance),  d2 = e^T P^-1 e
// Every symmetric block is computed on its upper triangle and mirrored, so S_kk, Sigma_kk and P are symmetric to the last bit.
// The chain factor, the sweeps, C and its factor, the row through Lc^-1 and the W^T W entry are pg_chain.h's, here as in the kernels.
#ifndef ALEGO_PG_COV_MATH_H_
#define ALEGO_PG_COV_MATH_H_
#include "../../include/alego_mi355x.h"
#include "pg_chain.h"
#include "pg_math.h"

// M = L^-1 of a lower-triangular 6x6 (row-major; the upper triangle of M is zero)
PG_FN void pgc_linv(const double* L, double* M) {
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      if (r < c) { M[r * 6 + c] = 0.0; continue; }
      double a = r == c ? 1.0 : 0.0;
#pragma unroll
      for (int p = c; p < r; ++p) a -= L[r * 6 + p] * M[p * 6 + c];
      M[r * 6 + c] = a / L[r * 6 + r];
    }
}
// D = M^T M for the lower-triangular M (= L^-T L^-1): entry (i, j) sums rows max(i, j) .. 5 in order, the same products both ways
PG_FN void pgc_mtm(const double* M, double* D) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      double a = 0.0;
#pragma unroll
      for (int p = j; p < 6; ++p) a += M[p * 6 + i] * M[p * 6 + j];
      D[i * 6 + j] = a; D[j * 6 + i] = a;
    }
}
// G = Lo M (M lower-triangular)
PG_FN void pgc_lom(const double* Lo, const double* M, double* G) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double a = 0.0;
#pragma unroll
      for (int p = c; p < 6; ++p) a += Lo[r * 6 + p] * M[p * 6 + c];
      G[r * 6 + c] = a;
    }
}
// the two products of one step of the backward recursion, one entry each (36 lanes of a wavefront, or two loops on the host):
// (S G)(a, j), then with Pm = S G the upper-triangle entry of G^T Pm that both (i, j) and (j, i) take
PG_FN double pgc_sg_entry(const double* S, const double* G, int a, int j) {
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < 6; ++b) s += S[a * 6 + b] * G[b * 6 + j];
  return s;
}
// entry (lo, hi) of G^T Pm, lo <= hi: S_kk(lo, hi) = S_kk(hi, lo) = D(lo, hi) + this
PG_FN double pgc_gtp_entry(const double* G, const double* Pm, int lo, int hi) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) s += G[a * 6 + lo] * Pm[a * 6 + hi];
  return s;
}

// P of a candidate from the blocks Sigma_ii, Sigma_jj, Sigma_ij (row-major; rows of node i, columns of node j), upper triangle mirrored
PG_FN void pgc_innovation(const double* A, const double* B, const double* Sii, const double* Sjj, const double* Sij, const double* var, double* P) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double t[12];   // row r of [A B] [[Sii, Sij], [Sij^T, Sjj]]
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) { a += A[r * 6 + k] * Sii[k * 6 + m]; b += A[r * 6 + k] * Sij[k * 6 + m]; }
#pragma unroll
      for (int k = 0; k < 6; ++k) { a += B[r * 6 + k] * Sij[m * 6 + k]; b += B[r * 6 + k] * Sjj[k * 6 + m]; }
      t[m] = a; t[6 + m] = b;
    }
#pragma unroll
    for (int c = r; c < 6; ++c) {
      double s = c == r ? var[r] : 0.0;
#pragma unroll
      for (int m = 0; m < 6; ++m) s += t[m] * A[c * 6 + m];
#pragma unroll
      for (int m = 0; m < 6; ++m) s += t[6 + m] * B[c * 6 + m];
      P[r * 6 + c] = s; P[c * 6 + r] = s;
    }
  }
}
// d2 = e^T P^-1 e by a 6x6 Cholesky; false when P is not finite or not positive definite (d2 is then 0)
PG_FN bool pgc_mahalanobis(const double* P, const double* e, double* d2) {
  double L[36], y[6];
  bool ok = pg_chol6(P, L);
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = e[i];
  pg_lsolve(L, y);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) s += y[i] * y[i];
  if (!(s >= 0.0) || !(s <= 1.79769313486231570815e+308)) ok = false;
  *d2 = ok ? s : 0.0;
  return ok;
}
// the unwhitened error of a candidate and its two Jacobian blocks at the poses xi, xj (pg_factor with variance 1)
PG_FN void pgc_candidate(const double* xi, const double* xj, const double* meas, double* e, double* A, double* B) {
  const double one[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
  pg_factor(xi, xj, meas, one, e, A, B);
}

// ---- the host twin: the same phases the device runs, in plain loops -------------------------------------------------------------
#include <cstring>
#include <vector>

struct PgcHost {
  int N = 0, NL = 0, n = 0;
  std::vector<double> Td, To, Z, C;   // L_kk, L_{k+1,k} [N][36]; W after pgc_host_factor: [N * 6][n]; Lc [n][n]
};
// the chain solve T x = b in place for one right-hand side b [N][6] whose entries before node k0 are zero; the backward sweep stops at node k1
inline void pgc_host_sweep(const PgcHost& H, double* x, int k0, int k1) {
  for (int k = k0; k < H.N; ++k) {
    double* y = x + (size_t)k * 6;
    pg_fwd_step(&H.Td[(size_t)k * 36], k > k0 ? &H.To[(size_t)(k - 1) * 36] : nullptr, k > k0 ? y - 6 : nullptr, y);
  }
  for (int k = H.N - 1; k >= k1; --k) {
    double* y = x + (size_t)k * 6;
    pg_bwd_step(&H.Td[(size_t)k * 36], k + 1 < H.N ? &H.To[(size_t)k * 36] : nullptr, y + 6, y);
  }
}
// linearise at poses12, factorise T along the chain, Z, the capacitance factor and W (pg_linearize .. pg_solve, then pgc_correct's
// substitution).  edges: the n_poses chain edges (edge 0 the prior, edge k: k - 1 -> k), then the loop edges.  ALEGO_ERR_ARG on a
// malformed graph.
inline int pgc_host_factor(const double* poses12, int N, const alego_graph_edge* edges, int n_edges, PgcHost* H) {
  if (!poses12 || N <= 0 || !edges || n_edges < N) return ALEGO_ERR_ARG;
  for (long i = 0; i < (long)N * 12; ++i) if (!pg_finite(poses12[i])) return ALEGO_ERR_ARG;
  for (int i = 0; i < n_edges; ++i) {
    const alego_graph_edge& e = edges[i];
    if (!(i < N ? pg_chain_ids(e.from, e.to, i) : pg_loop_ids(e.from, e.to, N)) || !pg_edge_finite(e.between, e.variance)) return ALEGO_ERR_ARG;
  }
  const int NL = n_edges - N, n = 6 * NL;
  H->N = N; H->NL = NL; H->n = n;
  std::vector<double> Jf((size_t)n_edges * 36), Jt((size_t)n_edges * 36);
  for (int i = 0; i < n_edges; ++i) {
    double r[6];
    pg_factor(edges[i].from < 0 ? nullptr : poses12 + (size_t)edges[i].from * 12, poses12 + (size_t)edges[i].to * 12, edges[i].between, edges[i].variance, r,
              &Jf[(size_t)i * 36], &Jt[(size_t)i * 36]);
  }
  H->Td.assign((size_t)N * 36, 0.0); H->To.assign((size_t)N * 36, 0.0);
  for (int k = 0; k < N; ++k) {
    pg_atb(&Jt[(size_t)k * 36], &Jt[(size_t)k * 36], &H->Td[(size_t)k * 36], false);
    if (k + 1 < N) {
      pg_atb(&Jf[(size_t)(k + 1) * 36], &Jf[(size_t)(k + 1) * 36], &H->Td[(size_t)k * 36], true);
      pg_atb(&Jt[(size_t)(k + 1) * 36], &Jf[(size_t)(k + 1) * 36], &H->To[(size_t)k * 36], false);
    }
  }
  // block Cholesky along the chain (pg_factor_chain): a bad pivot leaves NaN, as there
  double D[36];
  std::memcpy(D, H->Td.data(), sizeof(D));
  for (int k = 0; k < N; ++k) {
    double* Lk = &H->Td[(size_t)k * 36];
    pg_chol6(D, Lk);
    if (k + 1 == N) break;
    double* Lo = &H->To[(size_t)k * 36];
    pg_chain_lo(Lo, Lk, Lo);
    pg_chain_schur(&H->Td[(size_t)(k + 1) * 36], Lo, D);
  }
  H->Z.assign((size_t)N * 6 * n, 0.0); H->C.assign((size_t)n * n, 0.0);
  if (n == 0) return 0;
  // Z = T^-1 Jl^T, one column per row of a loop edge's Jacobian
  std::vector<double> x((size_t)N * 6);
  for (int c = 0; c < n; ++c) {
    const alego_graph_edge& e = edges[N + c / 6];
    std::fill(x.begin(), x.end(), 0.0);
    for (int i = 0; i < 6; ++i) { x[(size_t)e.from * 6 + i] = Jf[(size_t)(N + c / 6) * 36 + (c % 6) * 6 + i]; x[(size_t)e.to * 6 + i] = Jt[(size_t)(N + c / 6) * 36 + (c % 6) * 6 + i]; }
    pgc_host_sweep(*H, x.data(), 0, 0);
    for (int t = 0; t < N * 6; ++t) H->Z[(size_t)t * n + c] = x[t];
  }
  // C = I + Jl Z and its Cholesky factor (lower triangle, in place)
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      const alego_graph_edge& e = edges[N + a / 6];
      H->C[(size_t)a * n + b] = pg_cap_entry(a == b ? 1.0 : 0.0, &Jf[(size_t)(N + a / 6) * 36 + (a % 6) * 6], &H->Z[(size_t)e.from * 6 * n + b],
                                             &Jt[(size_t)(N + a / 6) * 36 + (a % 6) * 6], &H->Z[(size_t)e.to * 6 * n + b], n);
    }
  pg_chol_dense(H->C.data(), n, 0, 1, [] {});
  // W = rows of Z through Lc^-1, in place
  for (int t = 0; t < N * 6; ++t) pg_lc_row(H->C.data(), n, &H->Z[(size_t)t * n]);
  return 0;
}
// out (6x6) = (T^-1)_ab from the unit-column solutions col [6][N][6] of node b; pgc_host_sub_wtw then subtracts W_a^T W_b
inline void pgc_host_block(const PgcHost& H, const double* col, int a, double* out) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) out[r * 6 + c] = col[((size_t)c * H.N + a) * 6 + r];
}
inline void pgc_host_sub_wtw(const PgcHost& H, int a, int b, double* out) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      out[r * 6 + c] -= pg_wtw_entry(H.Z.data() + ((size_t)a * 6 + r) * H.n, H.Z.data() + ((size_t)b * 6 + c) * H.n, H.n);
    }
}
// the six unit-column solutions of node u: col [6][N][6] (entries of the nodes before `lo` are not computed)
inline void pgc_host_columns(const PgcHost& H, int u, int lo, std::vector<double>* col) {
  col->assign((size_t)6 * H.N * 6, 0.0);
  for (int c = 0; c < 6; ++c) {
    double* x = col->data() + (size_t)c * H.N * 6;
    x[(size_t)u * 6 + c] = 1.0;
    pgc_host_sweep(H, x, u, lo);
  }
}
// marg36 [N][36]: every marginal; pair36 [n_pairs][36]: Sigma_ij for pairs (i, j), rows of node i, columns of node j
inline int pgc_host_covariance(const double* poses12, int N, const alego_graph_edge* edges, int n_edges, const int* pairs, int n_pairs, double* marg36, double* pair36) {
  if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return ALEGO_ERR_ARG;
  for (int p = 0; p < n_pairs; ++p) if (pairs[2 * p] < 0 || pairs[2 * p] >= N || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= N) return ALEGO_ERR_ARG;
  PgcHost H;
  if (int r = pgc_host_factor(poses12, N, edges, n_edges, &H)) return r;
  if (marg36) {
    double S[36], D[36], G[36], M[36], Pm[36];
    for (int k = N - 1; k >= 0; --k) {
      pgc_linv(&H.Td[(size_t)k * 36], M);
      pgc_mtm(M, D);
      if (k + 1 < N) {
        pgc_lom(&H.To[(size_t)k * 36], M, G);
        for (int a = 0; a < 6; ++a) for (int j = 0; j < 6; ++j) Pm[a * 6 + j] = pgc_sg_entry(S, G, a, j);
        for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) { const int lo = i < j ? i : j, hi = i < j ? j : i; M[i * 6 + j] = D[lo * 6 + hi] + pgc_gtp_entry(G, Pm, lo, hi); }
        std::memcpy(S, M, sizeof(S));
      } else {
        std::memcpy(S, D, sizeof(S));
      }
      std::memcpy(marg36 + (size_t)k * 36, S, sizeof(S));
      pgc_host_sub_wtw(H, k, k, marg36 + (size_t)k * 36);
    }
  }
  std::vector<double> col;
  for (int p = 0; p < n_pairs && pair36; ++p) {
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    pgc_host_columns(H, j, i < j ? i : j, &col);
    pgc_host_block(H, col.data(), i, pair36 + (size_t)p * 36);
    pgc_host_sub_wtw(H, i, j, pair36 + (size_t)p * 36);
  }
  return 0;
}
// every candidate against the same graph: status 1 / -2, d2, the unwhitened error and P
inline int pgc_host_check(const double* poses12, int N, const alego_graph_edge* edges, int n_edges, const alego_graph_edge* cand, int n_cand, alego_graph_check* out) {
  if (n_cand < 0 || (n_cand > 0 && (!cand || !out))) return ALEGO_ERR_ARG;
  for (int c = 0; c < n_cand; ++c) {
    const alego_graph_edge& e = cand[c];
    if (!pg_loop_ids(e.from, e.to, N) || !pg_edge_finite(e.between, e.variance)) return ALEGO_ERR_ARG;
  }
  PgcHost H;
  if (int r = pgc_host_factor(poses12, N, edges, n_edges, &H)) return r;
  std::vector<double> ci, cj;
  for (int c = 0; c < n_cand; ++c) {
    const int i = cand[c].from, j = cand[c].to, lo = i < j ? i : j;
    double Sii[36], Sjj[36], Sij[36], A[36], B[36];
    pgc_host_columns(H, i, lo, &ci);
    pgc_host_columns(H, j, lo, &cj);
    pgc_host_block(H, ci.data(), i, Sii); pgc_host_sub_wtw(H, i, i, Sii);
    pgc_host_block(H, cj.data(), j, Sjj); pgc_host_sub_wtw(H, j, j, Sjj);
    pgc_host_block(H, cj.data(), i, Sij); pgc_host_sub_wtw(H, i, j, Sij);
    alego_graph_check& o = out[c];
    std::memset(&o, 0, sizeof(o));
    pgc_candidate(poses12 + (size_t)i * 12, poses12 + (size_t)j * 12, cand[c].between, o.error, A, B);
    pgc_innovation(A, B, Sii, Sjj, Sij, cand[c].variance, o.cov);
    o.status = pgc_mahalanobis(o.cov, o.error, &o.d2) ? 1 : -2;
  }
  return 0;
}
#endif
