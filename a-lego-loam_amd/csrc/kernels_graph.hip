// kernels_graph.hip — the key-pose graph of every slot, optimised on gfx950 (laserMapping.cpp:491-584).
//
// The graph of a slot: its archived key frames as Pose3 nodes, a prior on node 0, the odometry chain map_archive recorded
// (kernels_gmap.hip) and up to pg_loops_cap loop edges.  alego_graph_optimize runs plain Gauss-Newton in f64 for a chunk of slots
// at once; every phase is a kernel, a slot's work inside a phase never leaves its workgroup (or its lane):
//   pg_init        X <- Pose3(Rot3::RzRyRx, xyz) of the archived f32 key poses
//   pg_linearize   one lane per edge: whitened error and the two 6x6 Jacobian blocks (pg_math.h)
//   pg_assemble    one lane per node: the block-tridiagonal part T of J^T J (prior + chain) and the gradient g (chain + loops)
//   pg_factor      one lane per slot: block Cholesky of T along the chain, T = L L^T with L block-bidiagonal
//   pg_solve       one workgroup per slot, one lane per right-hand side: forward and backward sweeps of L for -g and for the 6 columns
//                  of every loop edge's Jacobian side by side; the loop terms enter exactly through the capacitance system
//                  C = I + J_loop T^-1 J_loop^T (Woodbury), factorised by the same workgroup; delta = z0 - Z C^-1 J_loop z0
//   pg_update      one workgroup per slot: |delta|_inf, the finiteness check, X <- X Expmap(delta), the stopping rule
//   pg_cost        one workgroup per slot: sum of squared whitened errors in a fixed order
//   pg_store       the estimate of a finished slot goes to LmCtx::pg_est
// All sums of a slot run in an order that depends on the slot's own graph only; the block arithmetic of pg_assemble, pg_factor_chain and
// pg_solve, with the order of every sum, is pg_chain.h (shared with kernels_pgcov.hip and the host twin).
// correctPoses (:561-584) for the slots that converged: pg_apply (poses, window reset words, map -> odom), then pg_retransform +
// the key-frame sort jobs once per resident frame (lm_host.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_cost.h"
#include "dev_copy.h"
#include "dev_mem.h"
#include "kf_store.h"
#include "pg_math.h"
#include "pg_work.h"
#include "pgraph.h"
#include "prof.h"

DEV_INLINE const alego_graph_edge* pg_edge_of(const LmCtx& L, int slot, int Nmax, int e) {
  return e < Nmax ? L.pg_chain + arc_row(L, slot, e) : L.pg_loops + (size_t)slot * L.pg_loops_cap + (e - Nmax);
}

__global__ void __launch_bounds__(PG_T) pg_init(LmCtx L, PgWork W) {
  const int q = blockIdx.y, k = blockIdx.x * PG_T + threadIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  if (k >= ctl[PC_N]) return;
  pg_from_pose6(arc_pose_of(L, ctl[PC_SLOT], k), W.X + ((size_t)q * W.Nmax + k) * 12);
}

// grid (edge tiles, chunk entries); force: also the slots that have finished (the final cost)
__global__ void __launch_bounds__(PG_T) pg_linearize(LmCtx L, PgWork W, int force) {
  const int q = blockIdx.y, e = blockIdx.x * PG_T + threadIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  if (ctl[PC_DONE] && !force) return;
  const int N = ctl[PC_N];
  if (!(e < N || (e >= W.Nmax && e < W.Nmax + ctl[PC_NL]))) return;
  const alego_graph_edge* ed = pg_edge_of(L, ctl[PC_SLOT], W.Nmax, e);
  const double* X = W.X + (size_t)q * W.Nmax * 12;
  const size_t o = (size_t)q * (W.Nmax + W.Lmax) + e;
  double r[6], Jf[36], Jt[36];
  pg_factor(ed->from < 0 ? nullptr : X + (size_t)ed->from * 12, X + (size_t)ed->to * 12, ed->between, ed->variance, r, Jf, Jt);
  for (int i = 0; i < 6; ++i) W.res[o * 6 + i] = r[i];
  for (int i = 0; i < 36; ++i) { W.Jf[o * 36 + i] = Jf[i]; W.Jt[o * 36 + i] = Jt[i]; }
}

// grid (node tiles, chunk entries): node k takes edge k (its `to` side), edge k + 1 (its `from` side) and, for the gradient, the loop
// edges in index order
__global__ void __launch_bounds__(PG_T) pg_assemble(LmCtx L, PgWork W) {
  const int q = blockIdx.y, k = blockIdx.x * PG_T + threadIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  if (ctl[PC_DONE]) return;
  const int N = ctl[PC_N], NL = ctl[PC_NL];
  if (k >= N) return;
  const size_t eb = (size_t)q * (W.Nmax + W.Lmax), nb = (size_t)q * W.Nmax + k;
  double D[36], gk[6] = {0, 0, 0, 0, 0, 0};
  pg_atb(W.Jt + (eb + k) * 36, W.Jt + (eb + k) * 36, D, false);
  pg_atr(W.Jt + (eb + k) * 36, W.res + (eb + k) * 6, gk);
  if (k + 1 < N) {
    double O[36];
    pg_atb(W.Jf + (eb + k + 1) * 36, W.Jf + (eb + k + 1) * 36, D, true);
    pg_atr(W.Jf + (eb + k + 1) * 36, W.res + (eb + k + 1) * 6, gk);
    pg_atb(W.Jt + (eb + k + 1) * 36, W.Jf + (eb + k + 1) * 36, O, false);   // H_{k+1,k}
    for (int i = 0; i < 36; ++i) W.To[nb * 36 + i] = O[i];
  }
  const alego_graph_edge* lp = L.pg_loops + (size_t)ctl[PC_SLOT] * L.pg_loops_cap;
  for (int l = 0; l < NL; ++l) {
    if (lp[l].from == k) pg_atr(W.Jf + (eb + W.Nmax + l) * 36, W.res + (eb + W.Nmax + l) * 6, gk);
    if (lp[l].to == k) pg_atr(W.Jt + (eb + W.Nmax + l) * 36, W.res + (eb + W.Nmax + l) * 6, gk);
  }
  for (int i = 0; i < 36; ++i) W.Td[nb * 36 + i] = D[i];
  for (int i = 0; i < 6; ++i) W.g[nb * 6 + i] = gk[i];
}

// one lane per chunk entry: the block Cholesky of T along the chain (pg_chain.h), D_0 = T_00.  pg_chol6's flag is not looked at: a pivot
// that is not positive gives NaN, which pg_update reports as a non-finite step.
__global__ void __launch_bounds__(64) pg_factor_chain(PgWork W) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= W.S) return;
  const int* ctl = W.ctl + q * PC_COUNT;
  if (ctl[PC_DONE]) return;
  const int N = ctl[PC_N];
  double* Td = W.Td + (size_t)q * W.Nmax * 36;
  double* To = W.To + (size_t)q * W.Nmax * 36;
  double D[36], Lk[36], Lo[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) D[i] = Td[i];
  for (int k = 0; k < N; ++k) {
    pg_chol6(D, Lk);
#pragma unroll
    for (int i = 0; i < 36; ++i) Td[(size_t)k * 36 + i] = Lk[i];
    if (k + 1 == N) break;
    pg_chain_lo(To + (size_t)k * 36, Lk, Lo);
#pragma unroll
    for (int i = 0; i < 36; ++i) To[(size_t)k * 36 + i] = Lo[i];
    pg_chain_schur(Td + (size_t)(k + 1) * 36, Lo, D);
  }
}

// grid (chunk entries), R lanes rounded up to wavefronts.  Lane 0 sweeps -g, lane 1 + 6 l + i row i of loop edge l's Jacobian
// (Jf at node `from`, Jt at node `to`, zero elsewhere).  Every lane reads the same factor blocks; its column of Z is its own.
__global__ void __launch_bounds__(PG_SOLVE_MAX) pg_solve(LmCtx L, PgWork W) {
  __shared__ double s_y[6 * ALEGO_GRAPH_MAX_LOOPS];
  const int q = blockIdx.x, c = threadIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  if (ctl[PC_DONE]) return;
  const int N = ctl[PC_N], NL = ctl[PC_NL], n = 6 * NL, R = W.R;
  const double* Td = W.Td + (size_t)q * W.Nmax * 36;
  const double* To = W.To + (size_t)q * W.Nmax * 36;
  double* g = W.g + (size_t)q * W.Nmax * 6;
  double* Z = W.Z + (size_t)q * W.Nmax * 6 * R;
  double* Cm = W.C + (size_t)q * 36 * W.Lmax * W.Lmax;
  const size_t eb = (size_t)q * (W.Nmax + W.Lmax) + W.Nmax;
  const alego_graph_edge* lp = L.pg_loops + (size_t)ctl[PC_SLOT] * L.pg_loops_cap;
  if (c < 1 + n) {
    const int l = c > 0 ? (c - 1) / 6 : 0, row = c > 0 ? (c - 1) % 6 : 0;
    const int from = c > 0 ? lp[l].from : -1, to = c > 0 ? lp[l].to : -1;
    const double* jf = W.Jf + (eb + l) * 36 + row * 6;
    const double* jt = W.Jt + (eb + l) * 36 + row * 6;
    double y[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < N; ++k) {   // forward
      double b[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) b[i] = c == 0 ? -g[k * 6 + i] : (k == from ? jf[i] : (k == to ? jt[i] : 0.0));
      pg_fwd_step(Td + (size_t)k * 36, k > 0 ? To + (size_t)(k - 1) * 36 : nullptr, y, b);
#pragma unroll
      for (int i = 0; i < 6; ++i) Z[((size_t)k * 6 + i) * R + c] = y[i] = b[i];
    }
    for (int k = N - 1; k >= 0; --k) {   // backward
      double b[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) b[i] = Z[((size_t)k * 6 + i) * R + c];
      pg_bwd_step(Td + (size_t)k * 36, k + 1 < N ? To + (size_t)k * 36 : nullptr, y, b);
#pragma unroll
      for (int i = 0; i < 6; ++i) Z[((size_t)k * 6 + i) * R + c] = y[i] = b[i];
    }
  }
  __syncthreads();
  if (NL > 0) {
    // capacitance C = I + J Z[:, 1:], right-hand side J z0: entry (a, b), a = (l, row), b = column 1 + b of Z (b = n: column 0)
    for (int t = c; t < n * (n + 1); t += blockDim.x) {
      const int a = t / (n + 1), b = t % (n + 1);
      const int l = a / 6, row = a % 6, col = b < n ? 1 + b : 0;
      const double s = pg_cap_entry(b == a ? 1.0 : 0.0, W.Jf + (eb + l) * 36 + row * 6, Z + (size_t)lp[l].from * 6 * R + col,
                                    W.Jt + (eb + l) * 36 + row * 6, Z + (size_t)lp[l].to * 6 * R + col, R);
      if (b < n) Cm[(size_t)a * n + b] = s; else s_y[a] = s;
    }
    __syncthreads();
    // dense Cholesky of C in place (lower triangle), then the two triangular solves for y, which only the optimiser needs
    pg_chol_dense(Cm, n, c, (int)blockDim.x, [] { __syncthreads(); });
    for (int j = 0; j < n; ++j) {
      if (c == 0) s_y[j] /= Cm[(size_t)j * n + j];
      __syncthreads();
      const double yj = s_y[j];
      for (int i = j + 1 + c; i < n; i += blockDim.x) s_y[i] -= Cm[(size_t)i * n + j] * yj;
      __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {
      if (c == 0) s_y[j] /= Cm[(size_t)j * n + j];
      __syncthreads();
      const double yj = s_y[j];
      for (int i = c; i < j; i += blockDim.x) s_y[i] -= Cm[(size_t)j * n + i] * yj;
      __syncthreads();
    }
  }
  // delta = z0 - Z[:, 1:] y, summed in column order
  for (int t = c; t < N * 6; t += blockDim.x) {
    const double* z = Z + (size_t)t * R;
    double s = z[0];
    for (int b = 0; b < n; ++b) s -= z[1 + b] * s_y[b];
    g[t] = s;
  }
}

// fixed-order workgroup sum / max over PG_T lanes
DEV_INLINE double pg_block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = PG_T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// grid (chunk entries): the step is taken only when every component of delta is finite (the state is left untouched otherwise)
__global__ void __launch_bounds__(PG_T) pg_update(PgWork W, int max_iters, double step_tol) {
  __shared__ double s_m[PG_T];
  __shared__ int s_bad;
  const int q = blockIdx.x;
  int* ctl = W.ctl + q * PC_COUNT;
  if (ctl[PC_DONE]) return;
  const int N = ctl[PC_N];
  const double* dl = W.g + (size_t)q * W.Nmax * 6;
  double* X = W.X + (size_t)q * W.Nmax * 12;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  double mx = 0.0;
  int bad = 0;
  for (int t = threadIdx.x; t < N * 6; t += PG_T) {
    const double a = fabs(dl[t]);
    if (!(a <= 1.79769313486231570815e+308)) bad = 1;
    mx = fmax(mx, a);
  }
  if (bad) s_bad = 1;
  s_m[threadIdx.x] = mx;
  __syncthreads();
  for (int h = PG_T / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) s_m[threadIdx.x] = fmax(s_m[threadIdx.x], s_m[threadIdx.x + h]);
    __syncthreads();
  }
  const double step = s_m[0];
  if (s_bad) {
    if (threadIdx.x == 0) { ctl[PC_STATUS] = -2; ctl[PC_DONE] = 1; }
    return;
  }
  for (int k = threadIdx.x; k < N; k += PG_T) {
    double E[12], O[12];
    pg_exp(dl + (size_t)k * 6, E);
    pg_compose(X + (size_t)k * 12, E, O);
    for (int i = 0; i < 12; ++i) X[(size_t)k * 12 + i] = O[i];
  }
  if (threadIdx.x == 0) {
    const int it = ctl[PC_ITERS] + 1;
    ctl[PC_ITERS] = it;
    W.dctl[q * PD_COUNT + PD_STEP] = step;
    if (step < step_tol) { ctl[PC_STATUS] = 2; ctl[PC_DONE] = 1; }
    else if (it >= max_iters) { ctl[PC_STATUS] = 1; ctl[PC_DONE] = 1; }
  }
}

// grid (chunk entries): which = PD_COST0 / PD_COST; lane t sums edges t, t + PG_T, ... (chain first, then loops), then a fixed tree
__global__ void __launch_bounds__(PG_T) pg_cost(PgWork W, int which) {
  __shared__ double s_m[PG_T];
  const int q = blockIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  const int N = ctl[PC_N], NL = ctl[PC_NL];
  const double* res = W.res + (size_t)q * (W.Nmax + W.Lmax) * 6;
  double s = 0.0;
  for (int e = threadIdx.x; e < N + NL; e += PG_T) {
    const double* r = res + (size_t)(e < N ? e : W.Nmax + (e - N)) * 6;
    for (int i = 0; i < 6; ++i) s += r[i] * r[i];
  }
  const double tot = pg_block_sum(s, s_m);
  if (threadIdx.x == 0) W.dctl[q * PD_COUNT + which] = tot;
}

__global__ void __launch_bounds__(PG_T) pg_store(LmCtx L, PgWork W) {
  const int q = blockIdx.y, t = blockIdx.x * PG_T + threadIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  if (ctl[PC_STATUS] < 1 || t >= ctl[PC_N] * 12) return;
  L.pg_est[arc_row(L, ctl[PC_SLOT], 0) * 12 + t] = W.X[(size_t)q * W.Nmax * 12 + t];
  if (t == 0) pg_stat_of(L, ctl[PC_SLOT])[PS_EST] = ctl[PC_N];
}

// ---- correctPoses (:561-584) for the slots with apply[slot] != 0 ------------------------------------------------------------
// grid (slots): archived poses and the resident ring's poses <- f32 pose of the estimate; recent_*.clear() as lm_host_reset_window sets it;
// map -> odom corrected by the last loop edge's ICP correction as lm_apply_correction does; loop_closed_ cleared
__global__ void __launch_bounds__(PG_T) pg_apply(LmCtx L, const int* apply) {
  const int slot = blockIdx.x;
  if (!apply[slot]) return;
  int* li = L.li + (size_t)slot * LI_COUNT;
  const int N = pg_stat_of(L, slot)[PS_EST], nkf = li[LI_NKF];
  for (int k = threadIdx.x; k < N; k += PG_T) {
    float kp[6];
    pg_to_pose6(L.pg_est + arc_row(L, slot, k) * 12, kp);
    float* ap = arc_pose_of(L, slot, k);
    for (int i = 0; i < 6; ++i) ap[i] = kp[i];
    if (k < nkf && k >= nkf - L.K) {
      float* rp = kf_pose_of(L, kf_row(L, slot, k));
      for (int i = 0; i < 6; ++i) rp[i] = kp[i];
    }
  }
  if (threadIdx.x == 0) {
    kf_reset_window([&](int w, int v) { li[w] = v; });
    double* ld = L.ld + (size_t)slot * LD_COUNT;
    dq_apply_correction(ld + LD_Q_M2O, ld + LD_T_M2O, L.pg_corr + (size_t)slot * 16);
    pg_stat_of(L, slot)[PS_CLOSED] = 0;
  }
}

// grid (8, 3, slots of the group): lm_store_kf's re-transform of ONE resident frame of every applied slot — the j-th oldest of its
// min(K, key frames) resident frames — from its raw clouds into kf_tmp_* for the key-frame sort jobs
__global__ void __launch_bounds__(PG_T) pg_retransform(LmCtx L, const int* apply, int slot0, int j) {
  const int slot = blockIdx.z + slot0, kind = blockIdx.y;
  if (!apply[slot]) return;
  int* li = L.li + (size_t)slot * LI_COUNT;
  const int nkf = li[LI_NKF], f = nkf - min(L.K, nkf) + j;
  if (f >= nkf) return;
  kf_row_to_tmp<PG_T>(L, slot, kf_entry(L, f), kind, false);
}
// the sort jobs ran: the frame is in its ring entry, the voxel lists of an applied slot no longer describe its window.  all: after the
// flush of the frames the last mapping frame left pending, every slot of the group is done with its sort (as map_update notes it), so the
// rounds that follow only sort the applied slots' frames
__global__ void pg_sorted(LmCtx L, const int* apply, int slot0, int n, int all) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  int* li = L.li + (size_t)(slot0 + s) * LI_COUNT;
  if (all || apply[slot0 + s]) li[LI_KF_PENDING] = 0;
  if (apply[slot0 + s]) li[LI_UVALID] = 0;
}

// ---- the optimiser's kernels and their grids, once each, for the W.S entries of a chunk ------------------------------------------
static void pg_launch_init(const LmCtx& L, const PgWork& W, hipStream_t st) {
  ALEGO_LAUNCH(pg_init, dim3((W.Nmax + PG_T - 1) / PG_T, W.S), dim3(PG_T), 0, st, L, W);
}
// errors and Jacobians at X (force: of the finished entries too); cost >= 0: then their squared sum into that double control word
static void pg_launch_linearize(const LmCtx& L, const PgWork& W, hipStream_t st, int force, int cost) {
  ALEGO_LAUNCH(pg_linearize, dim3((W.Nmax + W.Lmax + PG_T - 1) / PG_T, W.S), dim3(PG_T), 0, st, L, W, force);
  if (cost >= 0) ALEGO_LAUNCH(pg_cost, dim3(W.S), dim3(PG_T), 0, st, W, cost);
}
// T and g, the factor of T, the sweeps and the capacitance system: delta in g
static void pg_launch_solve(const LmCtx& L, const PgWork& W, hipStream_t st) {
  ALEGO_LAUNCH(pg_assemble, dim3((W.Nmax + PG_T - 1) / PG_T, W.S), dim3(PG_T), 0, st, L, W);
  ALEGO_LAUNCH(pg_factor_chain, dim3((W.S + 63) / 64), dim3(64), 0, st, W);
  ALEGO_LAUNCH(pg_solve, dim3(W.S), dim3(std::max(64, (W.R + 63) / 64 * 64)), 0, st, L, W);
}
void launch_pg_linear_pass(const LmCtx& L, const PgWork& W, hipStream_t st) {
  pg_launch_init(L, W, st);
  pg_launch_linearize(L, W, st, 0, -1);
  pg_launch_solve(L, W, st);
}
void launch_pg_apply(const LmCtx& L, const int* apply_dev, int n_slots, hipStream_t st) {
  ALEGO_LAUNCH(pg_apply, dim3(n_slots), dim3(PG_T), 0, st, L, apply_dev);
}
void launch_pg_retransform(const LmCtx& L, const int* apply_dev, int slot0, int n, int j, hipStream_t st) {
  ALEGO_LAUNCH(pg_retransform, dim3(8, 3, n), dim3(PG_T), 0, st, L, apply_dev, slot0, j);
}
void launch_pg_sorted(const LmCtx& L, const int* apply_dev, int slot0, int n, int all, hipStream_t st) {
  ALEGO_LAUNCH(pg_sorted, dim3((n + 63) / 64), dim3(64), 0, st, L, apply_dev, slot0, n, all);
}

// one loop edge per lane, at the index the host chose; the last entry of a slot leaves its correction and the loop count
__global__ void pg_append(LmCtx L, const PgAppend* a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  L.pg_loops[(size_t)a[i].slot * L.pg_loops_cap + a[i].index] = a[i].e;
  if (a[i].last) {
    for (int k = 0; k < 16; ++k) L.pg_corr[(size_t)a[i].slot * 16 + k] = a[i].corr[k];
    pg_stat_of(L, a[i].slot)[PS_LOOPS] = a[i].index + 1;
    pg_stat_of(L, a[i].slot)[PS_CLOSED] = 1;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
void graph_ctx_destroy(PgCtx* C) {
  if (!C) return;
  C->buf.clear(); C->apply.clear(); C->stage.clear();
  delete C;
}
void graph_ctx_set_budget(PgCtx** pc, long long bytes) {
  if (!*pc) *pc = new PgCtx();
  (*pc)->budget = std::max(1LL, bytes);
}

namespace {
// the counters of one slot: arc4 = LmCtx::arc_stat, pg4 = LmCtx::pg_stat
int pg_read_slot(const LmCtx& L, int slot, int* arc4, int* pg4, std::string* err) {
  return DevTry("graph", err).down(arc4, arc_stat_of(L, slot), AS_W).down(pg4, pg_stat_of(L, slot), PS_W);
}
}  // namespace

int graph_status(const LmCtx& L, int slot, int* out4, std::string* err) {
  int arc[AS_W], pg[PS_W];
  if (int r = pg_read_slot(L, slot, arc, pg, err)) return r;
  out4[0] = arc[AS_FRAMES]; out4[1] = pg[PS_LOOPS]; out4[2] = pg[PS_CLOSED]; out4[3] = pg[PS_EST];
  return 0;
}

int graph_get_edges(const LmCtx& L, int slot, int kind, int first, int n, alego_graph_edge* out, std::string* err) {
  int arc[AS_W], pg[PS_W];
  if (int r = pg_read_slot(L, slot, arc, pg, err)) return r;
  const int have = kind == 0 ? arc[AS_FRAMES] : pg[PS_LOOPS];
  if ((kind != 0 && kind != 1) || first < 0 || n < 0 || first > have || n > have - first || (n > 0 && !out)) return pg_fail(err, "graph_get_edges: range beyond the stored edges", ALEGO_ERR_ARG);
  if (n == 0) return 0;
  const alego_graph_edge* src = kind == 0 ? L.pg_chain + arc_row(L, slot, first) : L.pg_loops + (size_t)slot * L.pg_loops_cap + first;
  return DevTry("graph_get_edges", err, "copy").down(out, src, (size_t)n);
}

int graph_set_edges(const LmCtx& L, int slot, int first, int n, const alego_graph_edge* chain, std::string* err) {
  int arc[AS_W], pg[PS_W];
  if (int r = pg_read_slot(L, slot, arc, pg, err)) return r;
  const int have = arc[AS_FRAMES];
  if (first < 0 || n < 0 || first > have || n > have - first || (n > 0 && !chain)) return pg_fail(err, "graph_set_edges: range beyond the archived frames", ALEGO_ERR_ARG);
  for (int i = 0; i < n; ++i) {
    if (!pg_chain_ids(chain[i].from, chain[i].to, first + i)) return pg_fail(err, "graph_set_edges: chain edge i is the prior (from = -1, to = 0) or i - 1 -> i", ALEGO_ERR_ARG);
    if (!pg_edge_finite(chain[i].between, chain[i].variance)) return pg_fail(err, "graph_set_edges: measurement not finite or variance not positive and finite", ALEGO_ERR_ARG);
  }
  if (n == 0) return 0;
  return DevTry("graph_set_edges", err, "copy").up(L.pg_chain + arc_row(L, slot, first), chain, (size_t)n);
}

// appends every entry (validated as a whole first: nothing is written on an error)
int graph_append(PgCtx** pc, const LmCtx& L, int n_slots, const std::vector<PgAppend>& in, hipStream_t st, std::string* err) {
  if (in.empty()) return 0;
  if (!*pc) *pc = new PgCtx();
  PgCtx* C = *pc;
  std::vector<int> arc, pg;
  if (int r = pg_read_stats(L, n_slots, &arc, &pg, err)) return r;
  std::vector<PgAppend> a = in;
  std::vector<int> cnt(n_slots), last(n_slots, -1);
  for (int s = 0; s < n_slots; ++s) cnt[s] = pg[s * PS_W + PS_LOOPS];
  for (size_t i = 0; i < a.size(); ++i) {
    const alego_graph_edge& e = a[i].e;
    const int nf = arc[a[i].slot * AS_W + AS_FRAMES];
    if (!pg_loop_ids(e.from, e.to, nf)) return pg_fail(err, "graph: loop edge ids outside the archived frames, or from == to", ALEGO_ERR_ARG);
    if (!pg_edge_finite(e.between, e.variance)) return pg_fail(err, "graph: measurement not finite or variance not positive and finite", ALEGO_ERR_ARG);
    if (cnt[a[i].slot] >= L.pg_loops_cap) return pg_fail(err, "graph: max_loops loop edges are stored already", ALEGO_ERR_CAPACITY);
    a[i].index = cnt[a[i].slot]++;
    a[i].last = 0;
    last[a[i].slot] = (int)i;
  }
  for (int s = 0; s < n_slots; ++s) if (last[s] >= 0) a[last[s]].last = 1;
  DevTry c("graph", err);
  if (c.took(C->stage.reserve(a.size()), "staging allocation").at("append").up(C->stage.p, a)) return c;
  ALEGO_LAUNCH(pg_append, dim3(((int)a.size() + 63) / 64), dim3(64), 0, st, L, (const PgAppend*)C->stage.p, (int)a.size());
  return c.wait(st);
}

int graph_get_estimate(const LmCtx& L, int slot, int first, int n, double* poses12, std::string* err) {
  int arc[AS_W], pg[PS_W];
  if (int r = pg_read_slot(L, slot, arc, pg, err)) return r;
  const int have = pg[PS_EST];
  if (first < 0 || n < 0 || first > have || n > have - first || (n > 0 && !poses12)) return pg_fail(err, "graph_get_estimate: range beyond the poses of the last optimise", ALEGO_ERR_ARG);
  return DevTry("graph_get_estimate", err, "copy").down(poses12, L.pg_est + arc_row(L, slot, first) * 12, (size_t)n * 12);
}

// Gauss-Newton for the listed slots, chunk by chunk under the budget; out[i] belongs to slots[i].  apply_out[slot] = 1 for the slots whose
// correction is to be applied (converged, loop_closed_ set, opts.apply): the caller runs correctPoses for them.
int graph_optimize(PgCtx** pc, const LmCtx& L, int n_slots, const int* slots, int n, const alego_graph_opts& opt, alego_graph_result* out,
                   std::vector<int>* apply_out, hipStream_t st, std::string* err) {
  if (!*pc) *pc = new PgCtx();
  PgCtx* C = *pc;
  std::vector<int> arc, pg;
  if (int r = pg_read_stats(L, n_slots, &arc, &pg, err)) return r;
  apply_out->assign(n_slots, 0);
  std::vector<int> todo;
  PgPlan P;
  for (int i = 0; i < n; ++i) {
    const int s = slots[i];
    alego_graph_result& r = out[i];
    std::memset(&r, 0, sizeof(r));
    r.n_poses = arc[s * AS_W + AS_FRAMES]; r.n_loops = pg[s * PS_W + PS_LOOPS];
    if (arc[s * AS_W + AS_DROPPED] > 0) { r.status = -1; continue; }
    if (r.n_poses == 0) { r.status = 0; continue; }
    todo.push_back(i);
    P.cover(r.n_poses, r.n_loops);
  }
  if (todo.empty()) return 0;
  PgWork W;
  if (P.reserve(C, todo.size(), 16 * 256, [&](char* base, int S) { return pg_layout(&W, base, S, P.Nmax, P.Lmax); }) != hipSuccess)
    return pg_fail(err, "graph_optimize: scratch allocation failed (lower the budget or max_loops)", ALEGO_ERR_HIP);
  std::vector<int> ctl;
  std::vector<double> dctl;
  for (size_t c0 = 0; c0 < todo.size(); c0 += P.chunk) {
    const int S = (int)std::min<size_t>(P.chunk, todo.size() - c0);
    pg_layout(&W, C->buf.p, S, P.Nmax, P.Lmax);
    ctl.assign((size_t)S * PC_COUNT, 0);
    for (int q = 0; q < S; ++q) pg_ctl_entry(&ctl, q, out[todo[c0 + q]].n_poses, out[todo[c0 + q]].n_loops, slots[todo[c0 + q]]);
    DevTry c("graph_optimize", err, "upload");
    if (c.up(W.ctl, ctl, st) || c.took(hipMemsetAsync(W.dctl, 0, (size_t)S * PD_COUNT * sizeof(double), st))) return c;
    c.at("a kernel");
    pg_launch_init(L, W, st);
    for (int it = 0; it < opt.max_iters; ++it) {
      pg_launch_linearize(L, W, st, 0, it == 0 ? (int)PD_COST0 : -1);
      pg_launch_solve(L, W, st);
      ALEGO_LAUNCH(pg_update, dim3(S), dim3(PG_T), 0, st, W, opt.max_iters, opt.step_tol);
      // one read per iteration for the whole chunk: stop launching once every slot of it has finished
      if (c.down(ctl, W.ctl, st).wait(st)) return c;
      bool all = true;
      for (int q = 0; q < S; ++q) all = all && ctl[q * PC_COUNT + PC_DONE];
      if (all) break;
    }
    pg_launch_linearize(L, W, st, 1, (int)PD_COST);
    ALEGO_LAUNCH(pg_store, dim3((P.Nmax * 12 + PG_T - 1) / PG_T, S), dim3(PG_T), 0, st, L, W);
    dctl.assign((size_t)S * PD_COUNT, 0.0);
    if (c.down(ctl, W.ctl, st).down(dctl, W.dctl, st).wait(st)) return c;
    for (int q = 0; q < S; ++q) {
      alego_graph_result& r = out[todo[c0 + q]];
      const int s = slots[todo[c0 + q]];
      r.status = ctl[q * PC_COUNT + PC_STATUS]; r.iterations = ctl[q * PC_COUNT + PC_ITERS];
      r.cost0 = dctl[q * PD_COUNT + PD_COST0]; r.cost = dctl[q * PD_COUNT + PD_COST]; r.last_step = dctl[q * PD_COUNT + PD_STEP];
      if (r.status == 2 && opt.apply && pg[s * PS_W + PS_CLOSED]) { r.applied = 1; (*apply_out)[s] = 1; }
    }
  }
  return 0;
}

// the applied slots' flags on the device (kept with the context)
int graph_upload_apply(PgCtx* C, const std::vector<int>& apply, const int** dev, hipStream_t st, std::string* err) {
  if (int r = DevTry("graph_optimize", err).took(C->apply.reserve(apply.size())).at("upload").up(C->apply.p, apply, st).wait(st)) return r;
  *dev = C->apply.p;
  return 0;
}

// host only: the whitened errors and Jacobian blocks of pg_math.h for a list of edges over n_poses poses
int graph_residuals_host(const double* poses12, int n_poses, const alego_graph_edge* edges, int n_edges, double* whitened6, double* jac_from36, double* jac_to36) {
  for (int i = 0; i < n_edges; ++i) {
    const alego_graph_edge& e = edges[i];
    if (!pg_edge_ids(e.from, e.to, n_poses, -1) || !pg_edge_finite(e.between, e.variance)) return ALEGO_ERR_ARG;
  }
  for (int i = 0; i < n_edges; ++i) {
    const alego_graph_edge& e = edges[i];
    double r[6], Jf[36], Jt[36];
    pg_factor(e.from < 0 ? nullptr : poses12 + (size_t)e.from * 12, poses12 + (size_t)e.to * 12, e.between, e.variance, r, Jf, Jt);
    if (whitened6) std::memcpy(whitened6 + (size_t)i * 6, r, sizeof(r));
    if (jac_from36) std::memcpy(jac_from36 + (size_t)i * 36, Jf, sizeof(Jf));
    if (jac_to36) std::memcpy(jac_to36 + (size_t)i * 36, Jt, sizeof(Jt));
  }
  return 0;
}
