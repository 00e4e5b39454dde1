// pg_chain.h — the f64 block arithmetic of the key-pose graph's chain factor and of its sweeps (DESIGN.md sections 13 and 20), once each,
// for the optimiser (kernels_graph.hip), the covariance kernels (kernels_pgcov.hip) and the host twin (pg_cov_math.h) alike; tests/pg_cov_math/
// pg_cov_math_check.cpp holds every function against its plain statement, bit for bit.  Readable by a host compiler: plain pointers and
// numbers in, no runtime, no barrier of its own.  Blocks are 6x6, row-major.
//
// The order of every sum is the contract (the library is built with -ffp-contract=off, so the same operations give the same bits on the
// host and on the device) and stands on the function.  The copies this header replaced agreed in every order; no site keeps one of its own.
//   T = L L^T along the chain:  D_0 = T_00;  L_kk = chol(D_k)  (pg_chol6);  L_{k+1,k} = T_{k+1,k} L_kk^-T  (pg_chain_lo);
//                               D_{k+1} = T_{k+1,k+1} - L_{k+1,k} L_{k+1,k}^T  (pg_chain_schur)
//   T x = b:  y_k = L_kk^-1 (b_k - L_{k,k-1} y_{k-1})  (pg_fwd_step);  x_k = L_kk^-T (y_k - L_{k+1,k}^T x_{k+1})  (pg_bwd_step)
#ifndef ALEGO_PG_CHAIN_H_
#define ALEGO_PG_CHAIN_H_
#include <stddef.h>

#include "pg_math.h"

// out (+)= A^T B: entry (i, j) starts at out(i, j) (add) or 0 and takes A(k, i) B(k, j) for k = 0 .. 5 in order
PG_FN void pg_atb(const double* A, const double* B, double* out, bool add) {
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double a = add ? out[i * 6 + j] : 0.0;
      for (int k = 0; k < 6; ++k) a += A[k * 6 + i] * B[k * 6 + j];
      out[i * 6 + j] = a;
    }
}
// v += A^T r: component i starts at v(i) and takes A(k, i) r(k) for k = 0 .. 5 in order
PG_FN void pg_atr(const double* A, const double* r, double* v) {
  for (int i = 0; i < 6; ++i) {
    double a = v[i];
    for (int k = 0; k < 6; ++k) a += A[k * 6 + i] * r[k];
    v[i] = a;
  }
}

// L = chol(D), column by column: L(j, j) = sqrt(D(j, j) - L(j, p)^2 for p = 0 .. j - 1 in order), L(i, j) = (D(i, j) - L(i, p) L(j, p) for
// p = 0 .. j - 1 in order) / L(j, j); the upper triangle of L is zeroed, that of D is not read.  false when a pivot is not positive and
// finite: L then carries the NaN (or the infinity of a zero pivot) on, which is what pg_factor_chain wants (pg_update reports status -2).
PG_FN bool pg_chol6(const double* D, double* L) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = D[j * 6 + j];
#pragma unroll
    for (int p = 0; p < j; ++p) d -= L[j * 6 + p] * L[j * 6 + p];
    if (!(d > 0.0) || !(d <= 1.79769313486231570815e+308)) ok = false;
    d = sqrt(d);
    L[j * 6 + j] = d;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i < j) L[i * 6 + j] = 0.0;
      if (i > j) {
        double a = D[i * 6 + j];
#pragma unroll
        for (int p = 0; p < j; ++p) a -= L[i * 6 + p] * L[j * 6 + p];
        L[i * 6 + j] = a / d;
      }
    }
  }
  return ok;
}
// Lo = T Lk^-T: Lo(r, c) = (T(r, c) - Lo(r, j) Lk(c, j) for j = 0 .. c - 1 in order) / Lk(c, c).  T and Lo may be the same block.
PG_FN void pg_chain_lo(const double* T, const double* Lk, double* Lo) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double a = T[r * 6 + c];
#pragma unroll
      for (int j = 0; j < c; ++j) a -= Lo[r * 6 + j] * Lk[c * 6 + j];
      Lo[r * 6 + c] = a / Lk[c * 6 + c];
    }
}
// D = T - Lo Lo^T: D(r, c) = T(r, c) - Lo(r, j) Lo(c, j) for j = 0 .. 5 in order, all 36 entries (both triangles by the same products)
PG_FN void pg_chain_schur(const double* T, const double* Lo, double* D) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double a = T[r * 6 + c];
#pragma unroll
      for (int j = 0; j < 6; ++j) a -= Lo[r * 6 + j] * Lo[c * 6 + j];
      D[r * 6 + c] = a;
    }
}

// y <- Lk^-1 y, rows 0 .. 5: y(i) = (y(i) - Lk(i, j) y(j) for j = 0 .. i - 1 in order) / Lk(i, i)
PG_FN void pg_lsolve(const double* Lk, double* y) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = y[i];
#pragma unroll
    for (int j = 0; j < i; ++j) a -= Lk[i * 6 + j] * y[j];
    y[i] = a / Lk[i * 6 + i];
  }
}
// y <- Lk^-T y, rows 5 .. 0: y(i) = (y(i) - Lk(j, i) y(j) for j = i + 1 .. 5 in order) / Lk(i, i)
PG_FN void pg_ltsolve(const double* Lk, double* y) {
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double a = y[i];
#pragma unroll
    for (int j = i + 1; j < 6; ++j) a -= Lk[j * 6 + i] * y[j];
    y[i] = a / Lk[i * 6 + i];
  }
}
// one node of the forward sweep: y holds b_k and leaves y_k.  Lo = L_{k,k-1} with prev = y_{k-1}, or null where nothing couples (the first
// node of a sweep): y(i) -= Lo(i, j) prev(j) for j = 0 .. 5 in order, all six rows, then pg_lsolve.
PG_FN void pg_fwd_step(const double* Lk, const double* Lo, const double* prev, double* y) {
  if (Lo) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double a = y[i];
#pragma unroll
      for (int j = 0; j < 6; ++j) a -= Lo[i * 6 + j] * prev[j];
      y[i] = a;
    }
  }
  pg_lsolve(Lk, y);
}
// one node of the backward sweep: y holds y_k and leaves x_k.  Lo = L_{k+1,k} with next = x_{k+1}, or null at the last node:
// y(i) -= Lo(j, i) next(j) for j = 0 .. 5 in order, all six rows, then pg_ltsolve.
PG_FN void pg_bwd_step(const double* Lk, const double* Lo, const double* next, double* y) {
  if (Lo) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double a = y[i];
#pragma unroll
      for (int j = 0; j < 6; ++j) a -= Lo[j * 6 + i] * next[j];
      y[i] = a;
    }
  }
  pg_ltsolve(Lk, y);
}

// an entry of the capacitance system C = I + Jl Z (or of its right-hand side Jl z0): delta, then jf(j) zf(j) for j = 0 .. 5, then jt(j) zt(j)
// for j = 0 .. 5.  jf / jt: the row of the loop edge's two Jacobian blocks; zf / zt: the column of Z at the rows of its `from` / `to`
// node, `stride` apart.
PG_FN double pg_cap_entry(double delta, const double* jf, const double* zf, const double* jt, const double* zt, size_t stride) {
  double s = delta;
  for (int j = 0; j < 6; ++j) s += jf[j] * zf[(size_t)j * stride];
  for (int j = 0; j < 6; ++j) s += jt[j] * zt[(size_t)j * stride];
  return s;
}
// the lower Cholesky factor of the n x n matrix C in place, right-looking, shared among `lanes` workers that meet in sync() (the host:
// lane 0 of 1, a sync that does nothing).  Per column j: lane 0 takes the root of the pivot; C(i, j) /= pivot; then every C(i, k), j < k <= i,
// takes -= C(i, j) C(k, j) — so an entry receives its updates for j = 0, 1, ... in order whichever lane owns it.  The strict upper
// triangle is neither read nor written.  A pivot that is not positive leaves NaN.
template <class Sync>
PG_FN void pg_chol_dense(double* Cm, int n, int lane, int lanes, Sync sync) {
  for (int j = 0; j < n; ++j) {
    if (lane == 0) Cm[(size_t)j * n + j] = sqrt(Cm[(size_t)j * n + j]);
    sync();
    const double d = Cm[(size_t)j * n + j];
    for (int i = j + 1 + lane; i < n; i += lanes) Cm[(size_t)i * n + j] /= d;
    sync();
    const int m = n - j - 1;
    for (int t = lane; t < m * m; t += lanes) {
      const int i = j + 1 + t / m, k = j + 1 + t % m;
      if (k <= i) Cm[(size_t)i * n + k] -= Cm[(size_t)i * n + j] * Cm[(size_t)k * n + j];
    }
    sync();
  }
}
// a row z (n entries) of Z through Lc^-1 in place: z(j) = (z(j) - Lc(j, p) z(p) for p = 0 .. j - 1 in order) / Lc(j, j)
PG_FN void pg_lc_row(const double* Lc, int n, double* z) {
  for (int j = 0; j < n; ++j) {
    double a = z[j];
    for (int p = 0; p < j; ++p) a -= Lc[(size_t)j * n + p] * z[p];
    z[j] = a / Lc[(size_t)j * n + j];
  }
}
// (W_a^T W_b)(r, c) from row r of W_a and row c of W_b: wa(p) wb(p) for p = 0 .. n - 1 in order, from 0
PG_FN double pg_wtw_entry(const double* wa, const double* wb, int n) {
  double s = 0.0;
  for (int p = 0; p < n; ++p) s += wa[p] * wb[p];
  return s;
}

// ---- what an edge must be before it enters a graph ------------------------------------------------------------------------------
PG_FN bool pg_finite(double x) { return x - x == 0.0; }
// the measurement [12] finite, every variance [6] positive and finite
PG_FN bool pg_edge_finite(const double* between, const double* variance) {
  for (int k = 0; k < 12; ++k) if (!pg_finite(between[k])) return false;
  for (int k = 0; k < 6; ++k) if (!(variance[k] > 0.0) || !pg_finite(variance[k])) return false;
  return true;
}
// an edge among n poses: `to` in 0 .. n - 1, `from` in first .. n - 1, and different.  first = -1 lets a prior (from = -1) pass too
PG_FN bool pg_edge_ids(int from, int to, int n, int first) { return from >= first && to >= 0 && from < n && to < n && from != to; }
// a loop edge or a candidate: both ids among the poses
PG_FN bool pg_loop_ids(int from, int to, int n) { return pg_edge_ids(from, to, n, 0); }
// chain edge k is k - 1 -> k; the prior is chain edge 0 (from = -1)
PG_FN bool pg_chain_ids(int from, int to, int k) { return to == k && from == k - 1; }
#endif
