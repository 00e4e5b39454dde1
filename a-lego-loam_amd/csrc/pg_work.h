// pg_work.h — what kernels_graph.hip (the optimiser) and kernels_pgcov.hip (marginal covariances and the loop-edge
// gate, section 20) share: the chunk scratch of the key-pose graph, its control words, the context kept with the handle and the host
// helpers that size the scratch, cut a call into chunks, fill a chunk's control words and read a slot's counters.  The block arithmetic
// of the chain factor and its sweeps, and what an edge must be to enter a graph, is pg_chain.h.
#ifndef ALEGO_PG_WORK_H_
#define ALEGO_PG_WORK_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_copy.h"
#include "dev_mem.h"
#include "kf_store.h"
#include "pg_chain.h"
#include "pgraph.h"

#define PG_T 256                       // workgroup of the per-edge / per-node / per-slot-reduction kernels
#define PG_SOLVE_MAX 448               // lanes of pg_solve: 1 + 6 * ALEGO_GRAPH_MAX_LOOPS right-hand sides, rounded up to wavefronts
#define PG_BUDGET_DEFAULT (1LL << 30)  // bytes of chunk scratch
static_assert(1 + 6 * ALEGO_GRAPH_MAX_LOOPS <= PG_SOLVE_MAX, "pg_solve sweeps one right-hand side per lane");

// int control words of a chunk entry; PC_NC / PC_NU (candidate edges, their distinct nodes) are written by alego_graph_check_* only
enum { PC_STATUS = 0, PC_ITERS, PC_DONE, PC_N, PC_NL, PC_SLOT, PC_NC, PC_NU, PC_COUNT = 8 };
enum { PD_COST0 = 0, PD_COST, PD_STEP, PD_COUNT = 4 };                            // double control words

// the scratch of one chunk entry q lives at fixed strides (Nmax poses, Lmax loop edges, R = 1 + 6 Lmax right-hand sides)
struct PgWork {
  int S, Nmax, Lmax, R;
  int* ctl;        // [S][PC_COUNT]
  double* dctl;    // [S][PD_COUNT]
  double* X;       // [S][Nmax][12]
  double* res;     // [S][Nmax + Lmax][6]     edge e < Nmax: chain edge e (the prior is edge 0); Nmax + l: loop edge l
  double* Jf;      // [S][Nmax + Lmax][36]
  double* Jt;      // [S][Nmax + Lmax][36]
  double* Td;      // [S][Nmax][36]  diagonal blocks of T, then L_kk
  double* To;      // [S][Nmax][36]  T_{k+1,k}, then L_{k+1,k}
  double* g;       // [S][Nmax][6]   gradient, then delta
  double* Z;       // [S][Nmax][6][R]
  double* C;       // [S][6 Lmax][6 Lmax]
};

struct PgCtx {
  long long budget = PG_BUDGET_DEFAULT;
  DevBuf<char> buf;          // chunk scratch (pg_layout, then pgc_layout)
  DevBuf<int> apply;         // [n_slots]
  DevBuf<PgAppend> stage;    // loop edges on their way to pg_append
};

inline size_t pg_align(size_t b) { return (b + 255) & ~(size_t)255; }
// one array of a chunk layout: count elements at offset *o of base (base == nullptr: only the size is counted)
template <class T> inline void pg_take(char* base, size_t* o, T** p, size_t count) {
  if (base) *p = (T*)(base + *o);
  *o += pg_align(count * sizeof(T));
}
// bytes of a chunk of S entries; with base != nullptr the pointers are laid out too
inline size_t pg_layout(PgWork* W, char* base, int S, int Nmax, int Lmax) {
  size_t o = 0;
  const size_t s = (size_t)S, N = (size_t)Nmax, E = (size_t)Nmax + Lmax, R = 1 + 6 * (size_t)Lmax;
  W->S = S; W->Nmax = Nmax; W->Lmax = Lmax; W->R = (int)R;
  pg_take(base, &o, &W->ctl, s * PC_COUNT); pg_take(base, &o, &W->dctl, s * PD_COUNT); pg_take(base, &o, &W->X, s * N * 12);
  pg_take(base, &o, &W->res, s * E * 6); pg_take(base, &o, &W->Jf, s * E * 36); pg_take(base, &o, &W->Jt, s * E * 36);
  pg_take(base, &o, &W->Td, s * N * 36); pg_take(base, &o, &W->To, s * N * 36); pg_take(base, &o, &W->g, s * N * 6);
  pg_take(base, &o, &W->Z, s * N * 6 * R); pg_take(base, &o, &W->C, s * 36 * (size_t)Lmax * Lmax);
  return o;
}
// how a call is cut into chunks: the largest graph among its entries sizes every entry, the budget the entries of a chunk
struct PgPlan {
  int Nmax = 1, Lmax = 0, chunk = 0;
  void cover(int N, int NL) { Nmax = std::max(Nmax, N); Lmax = std::max(Lmax, NL); }
  // layout(base, S) -> bytes of a chunk of S entries; slack: what the alignment of one entry's arrays can add.  Reserves the scratch of a chunk.
  template <class F> hipError_t reserve(PgCtx* C, size_t entries, size_t slack, F layout) {
    const size_t per = layout(nullptr, 1) + slack;
    chunk = (int)std::max<long long>(1, std::min<long long>((long long)entries, C->budget / (long long)per));
    return C->buf.reserve(layout(nullptr, chunk));
  }
};
// the control words of a chunk on the host ([S][PC_COUNT], zero before): entry q's graph and candidates (the whole vector then goes to PgWork::ctl)
inline void pg_ctl_entry(std::vector<int>* ctl, int q, int N, int NL, int slot, int NC = 0, int NU = 0) {
  int* w = ctl->data() + (size_t)q * PC_COUNT;
  w[PC_N] = N; w[PC_NL] = NL; w[PC_SLOT] = slot; w[PC_NC] = NC; w[PC_NU] = NU;
}
inline int pg_fail(std::string* err, const char* msg, int rc) { *err = msg; return rc; }
// the counters of every slot: arc = LmCtx::arc_stat, pg = LmCtx::pg_stat
inline int pg_read_stats(const LmCtx& L, int n_slots, std::vector<int>* arc, std::vector<int>* pg, std::string* err) {
  arc->resize((size_t)n_slots * AS_W); pg->resize((size_t)n_slots * PS_W);
  return DevTry("graph", err).down(*arc, L.arc_stat).down(*pg, L.pg_stat);
}

// pg_init -> pg_linearize -> pg_assemble -> pg_factor_chain -> pg_solve once for the S entries of W (kernels_graph.hip): leaves the factor of
// T in Td / To, Z = T^-1 J_loop^T in columns 1 .. 6 loops of Z and the Cholesky factor of the capacitance matrix in C
void launch_pg_linear_pass(const LmCtx& L, const PgWork& W, hipStream_t st);
#endif
