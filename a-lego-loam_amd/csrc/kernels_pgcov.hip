// kernels_pgcov.hip — marginal covariances of the key-pose graph and the consistency of candidate loop edges on gfx950 (DESIGN.md
// section 20; what gtsam::Marginals is to a GTSAM user, laserMapping.h:9).
//
// One linear pass of the optimiser's kernels (pg_init .. pg_solve, kernels_graph.hip) at the archived poses leaves, per chunk entry, the
// block-bidiagonal factor of T, Z = T^-1 Jl^T and the Cholesky factor Lc of the capacitance matrix.  On top of it (pg_cov_math.h):
//   pgc_blocks    one lane per node: D_k = L_kk^-T L_kk^-1 and G_k = L_{k+1,k} L_kk^-1 — everything of the recursion that is not sequential
//   pgc_chain     one wavefront per slot, the 36 entries of a block on 36 lanes: S_kk = D_k + G_k^T S_{k+1,k+1} G_k backwards, operands through LDS
//   pgc_correct   one lane per (node, row): its row of Z through Lc^-1 in place (W), once for marginals and pairs; then Sigma_kk = S_kk - W_k^T W_k
//   pgc_columns   one workgroup per slot, one lane per unit column of the distinct nodes of its candidates: the chain solve side by side as
//                 pg_solve sweeps its own; then Sigma_ii, Sigma_jj, Sigma_ij of every candidate
//   pgc_check     one lane per candidate: error, Jacobian blocks, P, d2
// All sums of a slot run in an order fixed by its own graph: alone, in any order of the call and under any ALEGO_PG_BUDGET the outputs of a
// slot are bit-identical.  Nothing of a slot is written: the scratch is the optimiser's chunk scratch, extended.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_copy.h"
#include "dev_mem.h"
#include "kf_store.h"
#include "pg_cov_math.h"
#include "pg_work.h"
#include "pgraph.h"
#include "prof.h"

#define PGC_ROWS 192                                   // workgroup of pgc_correct: 32 nodes x 6 rows
#define PGC_COL_MAX (12 * ALEGO_GRAPH_MAX_LOOPS)       // lanes of pgc_columns: 6 unit columns for each of two nodes of every candidate

struct PgcCand { alego_graph_edge e; int ci, cj; };    // ci, cj: where from / to stand among the slot's distinct nodes

// the scratch the covariance kernels add to a chunk entry (Kmax candidates, Umax distinct nodes, Rc = 6 Umax unit columns)
struct PgCov {
  int Kmax, Umax, Rc, pad;
  double* Sd;               // [S][Nmax][36]  D_k, then S_kk, then Sigma_kk
  double* Gb;               // [S][Nmax][36]  G_k
  double* Y;                // [S][Nmax][6][Rc]
  int* nodes;               // [S][Umax]      ascending
  PgcCand* cand;            // [S][Kmax]
  double* blk;              // [S][Kmax][3][36]  Sigma_ii, Sigma_jj, Sigma_ij
  alego_graph_check* out;   // [S][Kmax]
};

// grid (node tiles, chunk entries)
__global__ void __launch_bounds__(PG_T) pgc_blocks(PgWork W, PgCov V) {
  const int q = blockIdx.y, k = blockIdx.x * PG_T + threadIdx.x;
  const int N = W.ctl[q * PC_COUNT + PC_N];
  if (k >= N) return;
  const size_t nb = ((size_t)q * W.Nmax + k) * 36;
  double Lk[36], M[36], D[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) Lk[i] = W.Td[nb + i];
  pgc_linv(Lk, M);
  pgc_mtm(M, D);
#pragma unroll
  for (int i = 0; i < 36; ++i) V.Sd[nb + i] = D[i];
  if (k + 1 == N) return;
#pragma unroll
  for (int i = 0; i < 36; ++i) Lk[i] = W.To[nb + i];
  pgc_lom(Lk, M, D);
#pragma unroll
  for (int i = 0; i < 36; ++i) V.Gb[nb + i] = D[i];
}

// grid (chunk entries), one wavefront: lane e < 36 owns entry (e / 6, e % 6) of the running block.  Per step the block and G_k go through
// LDS; G_{k-1} and D_{k-1} are fetched while step k computes.  Entry (i, j) takes the sum of (min, max): S stays symmetric to the last bit.
__global__ void __launch_bounds__(64) pgc_chain(PgWork W, PgCov V) {
  __shared__ double s_S[36], s_G[36], s_P[36];
  const int q = blockIdx.x, t = threadIdx.x;
  const int N = W.ctl[q * PC_COUNT + PC_N];
  const int e = t < 36 ? t : 0, r = e / 6, c = e % 6, lo = min(r, c), hi = max(r, c);
  double* Sd = V.Sd + (size_t)q * W.Nmax * 36;
  const double* Gb = V.Gb + (size_t)q * W.Nmax * 36;
#ifdef ALEGO_PGC_ONE_LANE
  // development build (ALEGO_EXTRA_FLAGS=-DALEGO_PGC_ONE_LANE, tools/pg_cov_timing.py): the same recursion on one lane, the shape of pg_factor_chain
  if (t == 0) {
    double S[36], G[36], Pm[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) S[i] = Sd[(size_t)(N - 1) * 36 + i];
    for (int k = N - 2; k >= 0; --k) {
#pragma unroll
      for (int i = 0; i < 36; ++i) G[i] = Gb[(size_t)k * 36 + i];
#pragma unroll
      for (int i = 0; i < 36; ++i) Pm[i] = pgc_sg_entry(S, G, i / 6, i % 6);
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) S[i * 6 + j] = S[j * 6 + i] = Sd[(size_t)k * 36 + i * 6 + j] + pgc_gtp_entry(G, Pm, i, j);
#pragma unroll
      for (int i = 0; i < 36; ++i) Sd[(size_t)k * 36 + i] = S[i];
    }
  }
  return;
#endif
  double s = Sd[(size_t)(N - 1) * 36 + e];
  double gn = 0.0, dn = 0.0;
  if (N > 1) { gn = Gb[(size_t)(N - 2) * 36 + e]; dn = Sd[(size_t)(N - 2) * 36 + lo * 6 + hi]; }
  for (int k = N - 2; k >= 0; --k) {
    if (t < 36) { s_S[e] = s; s_G[e] = gn; }
    const double d = dn;
    if (k > 0) { gn = Gb[(size_t)(k - 1) * 36 + e]; dn = Sd[(size_t)(k - 1) * 36 + lo * 6 + hi]; }
    __syncthreads();
    const double p = pgc_sg_entry(s_S, s_G, r, c);
    if (t < 36) s_P[e] = p;
    __syncthreads();
    s = d + pgc_gtp_entry(s_G, s_P, lo, hi);
    if (t < 36) Sd[(size_t)k * 36 + e] = s;
    __syncthreads();
  }
}

// grid (row tiles, chunk entries): lane (node k, row i).  marg: also Sigma_kk = S_kk - W_k^T W_k in place, lane (k, i) its row i; an entry
// that is not finite leaves status -2
__global__ void __launch_bounds__(PGC_ROWS) pgc_correct(PgWork W, PgCov V, int marg) {
  const int q = blockIdx.y, t = blockIdx.x * PGC_ROWS + threadIdx.x;
  int* ctl = W.ctl + q * PC_COUNT;
  const int N = ctl[PC_N], n = 6 * ctl[PC_NL], R = W.R;
  const bool on = t < N * 6;
  double* Z = W.Z + (size_t)q * W.Nmax * 6 * R;
  const double* Lc = W.C + (size_t)q * 36 * W.Lmax * W.Lmax;
  if (on) pg_lc_row(Lc, n, Z + (size_t)t * R + 1);
  if (!marg) return;
  __syncthreads();
  if (!on) return;
  const int k = t / 6;
  double* S = V.Sd + ((size_t)q * W.Nmax + k) * 36 + (t % 6) * 6;
  const double* wi = Z + (size_t)t * R + 1;
  bool bad = false;
  for (int c = 0; c < 6; ++c) {
    const double v = S[c] - pg_wtw_entry(wi, Z + ((size_t)k * 6 + c) * R + 1, n);
    S[c] = v;
    if (!(fabs(v) <= 1.79769313486231570815e+308)) bad = true;
  }
  if (bad) ctl[PC_STATUS] = -2;
}

// grid (chunk entries), 6 * (distinct nodes) lanes rounded up to wavefronts.  Lane c sweeps the unit column (nodes[c / 6], c % 6): forward
// from its own node (everything before is zero), backward down to the slot's smallest candidate node.  Every lane reads the same factor blocks.
__global__ void __launch_bounds__(PGC_COL_MAX) pgc_columns(PgWork W, PgCov V) {
  const int q = blockIdx.x, c = threadIdx.x;
  const int* ctl = W.ctl + q * PC_COUNT;
  const int N = ctl[PC_N], n = 6 * ctl[PC_NL], R = W.R, K = ctl[PC_NC], U = ctl[PC_NU], Rc = V.Rc;
  const double* Td = W.Td + (size_t)q * W.Nmax * 36;
  const double* To = W.To + (size_t)q * W.Nmax * 36;
  const double* Z = W.Z + (size_t)q * W.Nmax * 6 * R;
  const int* nodes = V.nodes + (size_t)q * V.Umax;
  double* Y = V.Y + (size_t)q * W.Nmax * 6 * Rc;
  if (c < 6 * U) {
    const int u = nodes[c / 6], row = c % 6, last = nodes[0];
    double y[6] = {0, 0, 0, 0, 0, 0};
    for (int k = u; k < N; ++k) {   // forward
      double b[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) b[i] = (k == u && i == row) ? 1.0 : 0.0;
      pg_fwd_step(Td + (size_t)k * 36, k > u ? To + (size_t)(k - 1) * 36 : nullptr, y, b);
#pragma unroll
      for (int i = 0; i < 6; ++i) Y[((size_t)k * 6 + i) * Rc + c] = y[i] = b[i];
    }
    for (int k = N - 1; k >= last; --k) {   // backward
      double b[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) b[i] = k >= u ? Y[((size_t)k * 6 + i) * Rc + c] : 0.0;
      pg_bwd_step(Td + (size_t)k * 36, k + 1 < N ? To + (size_t)k * 36 : nullptr, y, b);
#pragma unroll
      for (int i = 0; i < 6; ++i) Y[((size_t)k * 6 + i) * Rc + c] = y[i] = b[i];
    }
  }
  __syncthreads();
  // block w of candidate kc, entry (r, cc): (T^-1)_ab (r, cc) = component r at node a of the unit column (b, cc), minus (W_a^T W_b)(r, cc)
  for (int t = c; t < K * 108; t += blockDim.x) {
    const int kc = t / 108, w = (t / 36) % 3, r = (t % 36) / 6, cc = t % 6;
    const PgcCand& cd = V.cand[(size_t)q * V.Kmax + kc];
    const int a = w == 1 ? cd.e.to : cd.e.from, b = w == 0 ? cd.e.from : cd.e.to, col = w == 0 ? cd.ci : cd.cj;
    V.blk[(((size_t)q * V.Kmax + kc) * 3 + w) * 36 + r * 6 + cc] =
        Y[((size_t)a * 6 + r) * Rc + col * 6 + cc] - pg_wtw_entry(Z + ((size_t)a * 6 + r) * R + 1, Z + ((size_t)b * 6 + cc) * R + 1, n);
  }
}

// grid (candidate tiles, chunk entries), one lane per candidate
__global__ void __launch_bounds__(64) pgc_check(PgWork W, PgCov V) {
  const int q = blockIdx.y, kc = blockIdx.x * 64 + threadIdx.x;
  if (kc >= W.ctl[q * PC_COUNT + PC_NC]) return;
  const PgcCand& cd = V.cand[(size_t)q * V.Kmax + kc];
  const double* X = W.X + (size_t)q * W.Nmax * 12;
  const double* blk = V.blk + ((size_t)q * V.Kmax + kc) * 108;
  alego_graph_check* o = V.out + (size_t)q * V.Kmax + kc;
  double e[6], A[36], B[36];
  pgc_candidate(X + (size_t)cd.e.from * 12, X + (size_t)cd.e.to * 12, cd.e.between, e, A, B);
  pgc_innovation(A, B, blk, blk + 36, blk + 72, cd.e.variance, o->cov);
  double d2;
  const bool ok = pgc_mahalanobis(o->cov, e, &d2);
  o->status = ok ? 1 : -2; o->pad = 0; o->d2 = d2;
#pragma unroll
  for (int i = 0; i < 6; ++i) o->error[i] = e[i];
}

// ---- host -------------------------------------------------------------------------------------------------------------------
namespace {
size_t pgc_layout(PgCov* V, char* base, size_t o0, int S, int Nmax, int Kmax, int Umax, bool marg) {
  size_t o = o0;
  const size_t s = (size_t)S, N = (size_t)Nmax;
  V->Kmax = Kmax; V->Umax = Umax; V->Rc = 6 * Umax; V->pad = 0;
  pg_take(base, &o, &V->Sd, marg ? s * N * 36 : 0); pg_take(base, &o, &V->Gb, marg ? s * N * 36 : 0);
  pg_take(base, &o, &V->Y, s * N * 6 * (size_t)V->Rc); pg_take(base, &o, &V->nodes, s * Umax); pg_take(base, &o, &V->cand, s * Kmax);
  pg_take(base, &o, &V->blk, s * Kmax * 108); pg_take(base, &o, &V->out, s * Kmax);
  return o - o0;
}
struct PgcEntry { int slot, N, NL; std::vector<PgcCand> cand; std::vector<int> nodes, where; };   // where: the index of every candidate in the call

// the chunks of `ent` under the budget: the optimiser's linear pass, then the covariance kernels; after_chunk(W, V, first entry, S) reads results
template <class F>
int pgc_run(PgCtx** pc, const LmCtx& L, const std::vector<PgcEntry>& ent, bool marg, hipStream_t st, std::string* err, F after_chunk) {
  if (ent.empty()) return 0;
  if (!*pc) *pc = new PgCtx();
  PgCtx* C = *pc;
  PgPlan P;
  int Kmax = 0, Umax = 0;
  for (const PgcEntry& e : ent) {
    P.cover(e.N, e.NL); Kmax = std::max(Kmax, (int)e.cand.size()); Umax = std::max(Umax, (int)e.nodes.size());
  }
  const int Nmax = P.Nmax, Lmax = P.Lmax;
  PgWork W; PgCov V;
  auto layout = [&](char* base, int S) { const size_t a = pg_layout(&W, base, S, Nmax, Lmax); return a + pgc_layout(&V, base, a, S, Nmax, Kmax, Umax, marg); };
  if (P.reserve(C, ent.size(), 24 * 256, layout) != hipSuccess) return pg_fail(err, "graph covariance: scratch allocation failed (lower the budget)", ALEGO_ERR_HIP);
  std::vector<int> ctl, nodes;
  std::vector<PgcCand> cand;
  for (size_t c0 = 0; c0 < ent.size(); c0 += P.chunk) {
    const int S = (int)std::min<size_t>(P.chunk, ent.size() - c0);
    layout(C->buf.p, S);
    ctl.assign((size_t)S * PC_COUNT, 0);
    nodes.assign((size_t)S * std::max(Umax, 1), 0);
    cand.assign((size_t)S * std::max(Kmax, 1), PgcCand());
    for (int q = 0; q < S; ++q) {
      const PgcEntry& e = ent[c0 + q];
      pg_ctl_entry(&ctl, q, e.N, e.NL, e.slot, (int)e.cand.size(), (int)e.nodes.size());
      std::copy(e.nodes.begin(), e.nodes.end(), nodes.begin() + (size_t)q * Umax);
      std::copy(e.cand.begin(), e.cand.end(), cand.begin() + (size_t)q * Kmax);
    }
    // (nodes and cand keep one spare element when there are no candidates: Kmax == 0 means Umax == 0, and nothing is copied)
    if (int r = DevTry("graph covariance", err).up(W.ctl, ctl, st).up(V.nodes, nodes.data(), (size_t)S * Umax, st).up(V.cand, cand.data(), (size_t)S * Kmax, st)) return r;
    launch_pg_linear_pass(L, W, st);
    if (marg) {
      ALEGO_LAUNCH(pgc_blocks, dim3((Nmax + PG_T - 1) / PG_T, S), dim3(PG_T), 0, st, W, V);
      ALEGO_LAUNCH(pgc_chain, dim3(S), dim3(64), 0, st, W, V);
    }
    if (marg || Lmax > 0) ALEGO_LAUNCH(pgc_correct, dim3((Nmax * 6 + PGC_ROWS - 1) / PGC_ROWS, S), dim3(PGC_ROWS), 0, st, W, V, marg ? 1 : 0);
    if (Kmax > 0) {
      ALEGO_LAUNCH(pgc_columns, dim3(S), dim3(std::max(64, (V.Rc + 63) / 64 * 64)), 0, st, W, V);
      ALEGO_LAUNCH(pgc_check, dim3((Kmax + 63) / 64, S), dim3(64), 0, st, W, V);
    }
    if (int r = after_chunk(W, V, c0, S)) return r;
  }
  return 0;
}
}  // namespace

int graph_marginals(PgCtx** pc, const LmCtx& L, int n_slots, const int* slots, int n, int cap, double* cov36, alego_graph_cov_result* out, hipStream_t st,
                    std::string* err) {
  std::vector<int> arc, pg;
  if (int r = pg_read_stats(L, n_slots, &arc, &pg, err)) return r;
  std::vector<PgcEntry> ent;
  std::vector<int> which;
  for (int i = 0; i < n; ++i) {
    const int s = slots[i];
    alego_graph_cov_result& r = out[i];
    std::memset(&r, 0, sizeof(r));
    r.n_poses = arc[s * AS_W + AS_FRAMES]; r.n_loops = pg[s * PS_W + PS_LOOPS];
    if (arc[s * AS_W + AS_DROPPED] > 0) { r.status = -1; continue; }
    if (r.n_poses == 0) continue;
    PgcEntry e; e.slot = s; e.N = r.n_poses; e.NL = r.n_loops;
    ent.push_back(e); which.push_back(i);
  }
  std::vector<int> ctl;
  std::vector<double> host;
  return pgc_run(pc, L, ent, true, st, err, [&](const PgWork& W, const PgCov& V, size_t c0, int S) {
    ctl.resize((size_t)S * PC_COUNT); host.resize((size_t)S * W.Nmax * 36);
    if (int r = DevTry("graph_marginals", err, "a kernel").down(ctl, W.ctl, st).down(host, V.Sd, st).wait(st)) return r;
    for (int q = 0; q < S; ++q) {
      const int i = which[c0 + q];
      out[i].status = ctl[(size_t)q * PC_COUNT + PC_STATUS] == -2 ? -2 : 1;
      std::memcpy(cov36 + (size_t)i * cap * 36, host.data() + (size_t)q * W.Nmax * 36, (size_t)std::min(out[i].n_poses, cap) * 36 * sizeof(double));
    }
    return 0;
  });
}

// active[i] == 0: candidate i is not judged (status 0).  Every other candidate is validated as alego_graph_add_edge validates an edge.
int graph_check(PgCtx** pc, const LmCtx& L, int n_slots, const int* slots, int n, const alego_graph_edge* e, const char* active, alego_graph_check* out,
                hipStream_t st, std::string* err) {
  std::vector<int> arc, pg;
  if (int r = pg_read_stats(L, n_slots, &arc, &pg, err)) return r;
  std::vector<int> entry_of(n_slots, -1);
  std::vector<PgcEntry> ent;
  for (int i = 0; i < n; ++i) {
    std::memset(&out[i], 0, sizeof(out[i]));
    if (active && !active[i]) continue;
    const int s = slots[i], nf = arc[s * AS_W + AS_FRAMES];
    if (!pg_loop_ids(e[i].from, e[i].to, nf)) return pg_fail(err, "graph check: edge ids outside the archived frames, or from == to", ALEGO_ERR_ARG);
    if (!pg_edge_finite(e[i].between, e[i].variance)) return pg_fail(err, "graph check: measurement not finite or variance not positive and finite", ALEGO_ERR_ARG);
    if (entry_of[s] < 0) {
      entry_of[s] = (int)ent.size();
      PgcEntry x; x.slot = s; x.N = nf; x.NL = pg[s * PS_W + PS_LOOPS];
      ent.push_back(x);
    }
    PgcEntry& x = ent[entry_of[s]];
    if ((int)x.cand.size() >= ALEGO_GRAPH_MAX_LOOPS) return pg_fail(err, "graph check: more than ALEGO_GRAPH_MAX_LOOPS candidates for one slot", ALEGO_ERR_CAPACITY);
    PgcCand c; c.e = e[i]; c.ci = c.cj = 0;
    x.cand.push_back(c); x.where.push_back(i);
  }
  std::vector<PgcEntry> run;
  for (PgcEntry& x : ent) {
    if (arc[x.slot * AS_W + AS_DROPPED] > 0) { for (int i : x.where) out[i].status = -1; continue; }
    for (const PgcCand& c : x.cand) { x.nodes.push_back(c.e.from); x.nodes.push_back(c.e.to); }
    std::sort(x.nodes.begin(), x.nodes.end());
    x.nodes.erase(std::unique(x.nodes.begin(), x.nodes.end()), x.nodes.end());
    for (PgcCand& c : x.cand) {
      c.ci = (int)(std::lower_bound(x.nodes.begin(), x.nodes.end(), c.e.from) - x.nodes.begin());
      c.cj = (int)(std::lower_bound(x.nodes.begin(), x.nodes.end(), c.e.to) - x.nodes.begin());
    }
    run.push_back(std::move(x));
  }
  std::vector<alego_graph_check> host;
  return pgc_run(pc, L, run, false, st, err, [&](const PgWork&, const PgCov& V, size_t c0, int S) {
    host.resize((size_t)S * V.Kmax);
    if (int r = DevTry("graph check", err, "a kernel").down(host, V.out, st).wait(st)) return r;
    for (int q = 0; q < S; ++q) {
      const PgcEntry& x = run[c0 + q];
      for (size_t k = 0; k < x.where.size(); ++k) out[x.where[k]] = host[(size_t)q * V.Kmax + k];
    }
    return 0;
  });
}

int graph_covariance_host(const double* poses12, int n_poses, const alego_graph_edge* edges, int n_edges, const int* pairs, int n_pairs, double* marg36, double* pair36) {
  return pgc_host_covariance(poses12, n_poses, edges, n_edges, pairs, n_pairs, marg36, pair36);
}
int graph_check_host(const double* poses12, int n_poses, const alego_graph_edge* edges, int n_edges, const alego_graph_edge* cand, int n_cand, alego_graph_check* out) {
  return pgc_host_check(poses12, n_poses, edges, n_edges, cand, n_cand, out);
}
