// Stand-alone run of csrc/pg_cov_math.h, the arithmetic of the key-pose graph's marginal covariances and of the loop-edge gate that the device
// kernels and the host twin share (tests/test_graph_cov.py builds it with -fsanitize=address,undefined, writes the cases and compares the
// output with numpy's dense inverse).  The header must be readable by a host compiler without the HIP runtime.
//
//   pg_cov_math_check CASES   CASES: per case, every real number as a C99 hexadecimal float (exact in both directions):
//                               n_poses n_edges n_pairs n_cand / poses[n_poses][12] / per edge: from to between[12] variance[6] (chain first) /
//                               per pair: i j / per candidate: from to between[12] variance[6]
//   prints per case           marginals[n_poses][36]  pairs[n_pairs][36]  per candidate: status d2 error[6] P[36];  "pg_cov_math ok <cases>" at the end
//
// Before the cases: every function of csrc/pg_chain.h against its plain statement written out below, bit for bit (chain_checks; its count goes
// to stderr as "pg_chain ok <checks>", a difference ends the program with status 1).
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pg_cov_math.h"

// ---- csrc/pg_chain.h against plain statements ----------------------------------------------------------------------------------
static int g_checks = 0;
static bool fail(const char* what, int i) { std::fprintf(stderr, "pg_chain: %s differs (case %d)\n", what, i); return false; }
// equal as bits, or NaN on both sides (the sign and payload of a NaN are the compiler's to choose)
static bool same(const double* a, const double* b, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (std::memcmp(a + i, b + i, sizeof(double)) != 0 && !(a[i] != a[i] && b[i] != b[i])) return false;
  ++g_checks;
  return true;
}
static unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
static double rnd() {   // uniform in (-1, 1)
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(long long)(g_seed >> 11) / 4503599627370496.0 - 1.0;
}
static void rnd_block(double* A) { for (int i = 0; i < 36; ++i) A[i] = rnd(); }
static void rnd_spd(double* D, double shift) {   // A A^T + shift I
  double A[36];
  rnd_block(A);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) { double s = i == j ? shift : 0.0; for (int k = 0; k < 6; ++k) s += A[i * 6 + k] * A[j * 6 + k]; D[i * 6 + j] = s; }
}
// L L^T = D, lower, column by column
static bool ref_chol6(const double* D, double* L) {
  bool ok = true;
  for (int i = 0; i < 36; ++i) L[i] = 0.0;
  for (int j = 0; j < 6; ++j) {
    double d = D[j * 6 + j];
    for (int p = 0; p < j; ++p) d -= L[j * 6 + p] * L[j * 6 + p];
    ok = ok && d > 0.0 && d <= std::numeric_limits<double>::max();
    L[j * 6 + j] = std::sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double a = D[i * 6 + j];
      for (int p = 0; p < j; ++p) a -= L[i * 6 + p] * L[j * 6 + p];
      L[i * 6 + j] = a / L[j * 6 + j];
    }
  }
  return ok;
}
static bool check_chol6(const double* D, bool want_ok, bool want_nan, const char* what, int i) {
  double L[36], Lr[36];
  for (double& v : L) v = 7.0;   // the upper triangle must be written
  const bool ok = pg_chol6(D, L), okr = ref_chol6(D, Lr);
  bool nan = false;
  for (double v : L) nan = nan || v != v;
  if (ok != want_ok || okr != want_ok || nan != want_nan || !same(L, Lr, 36)) return fail(what, i);
  return true;
}
static void ref_serial_chol(std::vector<double>* C, int n) {
  double* Cm = C->data();
  for (int j = 0; j < n; ++j) {
    Cm[(size_t)j * n + j] = std::sqrt(Cm[(size_t)j * n + j]);
    for (int i = j + 1; i < n; ++i) Cm[(size_t)i * n + j] /= Cm[(size_t)j * n + j];
    for (int i = j + 1; i < n; ++i)
      for (int k = j + 1; k <= i; ++k) Cm[(size_t)i * n + k] -= Cm[(size_t)i * n + j] * Cm[(size_t)k * n + j];
  }
}
// pg_chol_dense on `lanes` lanes that run ONE AT A TIME in lane order between barriers: a lane is a thread that holds the baton while it runs
// and hands it to the next lane in sync(), so every lane has finished a phase before any lane starts the next
static void laned_chol(std::vector<double>* C, int n, int lanes) {
  std::mutex m;
  std::vector<std::condition_variable> cv(lanes);
  int turn = 0;
  std::vector<std::thread> th;
  for (int lane = 0; lane < lanes; ++lane)
    th.emplace_back([&, lane] {
      std::unique_lock<std::mutex> lk(m);
      auto mine = [&] { cv[lane].wait(lk, [&] { return turn == lane; }); };
      auto pass = [&] { turn = (lane + 1) % lanes; cv[turn].notify_one(); };
      mine();
      pg_chol_dense(C->data(), n, lane, lanes, [&] { if (lanes > 1) { pass(); mine(); } });
      pass();
    });
  for (std::thread& t : th) t.join();
}

static bool chain_checks() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double A[36], B[36], D[36], L[36], Lo[36], Lor[36], S[36], Sr[36], v[6], vr[6], r[6];
  for (int t = 0; t < 200; ++t) {
    // pg_atb / pg_atr
    rnd_block(A); rnd_block(B); rnd_block(S);
    for (int i = 0; i < 6; ++i) r[i] = rnd();
    for (int add = 0; add < 2; ++add) {
      for (int i = 0; i < 36; ++i) Sr[i] = S[i];
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { double s = add ? Sr[i * 6 + j] : 0.0; for (int k = 0; k < 6; ++k) s += A[k * 6 + i] * B[k * 6 + j]; Sr[i * 6 + j] = s; }
      std::memcpy(D, S, sizeof(D));
      pg_atb(A, B, D, add != 0);
      if (!same(D, Sr, 36)) return fail("pg_atb", t);
    }
    for (int i = 0; i < 6; ++i) { v[i] = vr[i] = rnd(); }
    for (int i = 0; i < 6; ++i) for (int k = 0; k < 6; ++k) vr[i] += A[k * 6 + i] * r[k];
    pg_atr(A, r, v);
    if (!same(v, vr, 6)) return fail("pg_atr", t);
    // pg_chol6 on a random SPD block
    rnd_spd(D, 0.5);
    if (!check_chol6(D, true, false, "pg_chol6", t)) return false;
    // a chain step: L_kk = chol(D_k), L_{k+1,k} = T_{k+1,k} L_kk^-T, D_{k+1} = T_{k+1,k+1} - L_{k+1,k} L_{k+1,k}^T
    pg_chol6(D, L);
    rnd_block(A); rnd_spd(B, 40.0);
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 6; ++c) { double a = A[rr * 6 + c]; for (int j = 0; j < c; ++j) a -= Lor[rr * 6 + j] * L[c * 6 + j]; Lor[rr * 6 + c] = a / L[c * 6 + c]; }
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 6; ++c) { double a = B[rr * 6 + c]; for (int j = 0; j < 6; ++j) a -= Lor[rr * 6 + j] * Lor[c * 6 + j]; Sr[rr * 6 + c] = a; }
    pg_chain_lo(A, L, Lo);
    pg_chain_schur(B, Lo, S);
    if (!same(Lo, Lor, 36) || !same(S, Sr, 36)) return fail("chain step", t);
    pg_chain_lo(A, L, A);   // in place, as the host twin calls it
    if (!same(A, Lor, 36)) return fail("chain step in place", t);
    // the factor reproduces its block: L_{k+1,k} L_kk^T = T_{k+1,k} to rounding (the formulas above are the right ones)
    rnd_block(B);
    pg_chain_lo(B, L, Lo);
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
        for (int j = 0; j < 6; ++j) s += Lo[rr * 6 + j] * L[c * 6 + j];
        if (std::fabs(s - B[rr * 6 + c]) > 1e-12) return fail("chain step product", t);
      }
    // forward and backward steps, with and without the coupling block
    for (int cpl = 0; cpl < 2; ++cpl) {
      double b[6], o[6], y[6], yr[6];
      for (int i = 0; i < 6; ++i) { b[i] = rnd(); o[i] = rnd(); }
      for (int i = 0; i < 6; ++i) { double a = b[i]; if (cpl) for (int j = 0; j < 6; ++j) a -= Lo[i * 6 + j] * o[j]; yr[i] = a; }
      for (int i = 0; i < 6; ++i) { double a = yr[i]; for (int j = 0; j < i; ++j) a -= L[i * 6 + j] * yr[j]; yr[i] = a / L[i * 6 + i]; }
      std::memcpy(y, b, sizeof(y));
      pg_fwd_step(L, cpl ? Lo : nullptr, cpl ? o : nullptr, y);
      if (!same(y, yr, 6)) return fail("pg_fwd_step", t * 2 + cpl);
      for (int i = 0; i < 6; ++i) { double a = b[i]; if (cpl) for (int j = 0; j < 6; ++j) a -= Lo[j * 6 + i] * o[j]; yr[i] = a; }
      for (int i = 5; i >= 0; --i) { double a = yr[i]; for (int j = i + 1; j < 6; ++j) a -= L[j * 6 + i] * yr[j]; yr[i] = a / L[i * 6 + i]; }
      std::memcpy(y, b, sizeof(y));
      pg_bwd_step(L, cpl ? Lo : nullptr, cpl ? o : nullptr, y);
      if (!same(y, yr, 6)) return fail("pg_bwd_step", t * 2 + cpl);
    }
    // a capacitance entry, a row through Lc^-1, a W^T W entry (strided and dense operands)
    const int n = 1 + t % 13;
    std::vector<double> Z((size_t)12 * n), Lc((size_t)n * n), z(n), zr(n);
    for (double& x : Z) x = rnd();
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) Lc[(size_t)i * n + j] = i == j ? 2.0 + rnd() : rnd();
    const int col = t % n;
    double s = t % 2 ? 1.0 : 0.0;
    for (int j = 0; j < 6; ++j) s += A[j] * Z[(size_t)j * n + col];
    for (int j = 0; j < 6; ++j) s += B[j] * Z[(size_t)(6 + j) * n + col];
    const double got = pg_cap_entry(t % 2 ? 1.0 : 0.0, A, &Z[col], B, &Z[(size_t)6 * n + col], n);
    if (!same(&got, &s, 1)) return fail("pg_cap_entry", t);
    for (int j = 0; j < n; ++j) z[j] = zr[j] = rnd();
    for (int j = 0; j < n; ++j) { double a = zr[j]; for (int p = 0; p < j; ++p) a -= Lc[(size_t)j * n + p] * zr[p]; zr[j] = a / Lc[(size_t)j * n + j]; }
    pg_lc_row(Lc.data(), n, z.data());
    if (!same(z.data(), zr.data(), n)) return fail("pg_lc_row", t);
    double w = 0.0;
    for (int p = 0; p < n; ++p) w += Z[p] * Z[(size_t)n + p];
    const double gw = pg_wtw_entry(&Z[0], &Z[n], n);
    if (!same(&gw, &w, 1)) return fail("pg_wtw_entry", t);
  }
  // pg_chol6: a zero pivot, a negative pivot, an infinite entry off the diagonal — the flag is false and the NaN is carried on to the last
  // pivot; an infinite first pivot — the flag is false though no NaN arises (its column is x / inf = 0)
  for (int t = 0; t < 4; ++t) {
    rnd_spd(D, 0.5);
    if (t == 0) { for (int i = 0; i < 6; ++i) D[1 * 6 + i] = D[i * 6 + 1] = 0.0; }
    if (t == 1) D[2 * 6 + 2] = -1.0;
    if (t == 2) D[3 * 6 + 1] = D[1 * 6 + 3] = inf;
    if (t == 3) D[0] = inf;
    if (!check_chol6(D, false, t < 3, "pg_chol6 at a bad pivot", t)) return false;
    pg_chol6(D, L);
    if (t < 3 ? L[35] == L[35] : L[0] != inf) return fail("pg_chol6: what a bad pivot leaves", t);
  }
  // the dense Cholesky on 1, 3 and 64 lanes against the serial loop
  for (int n : {0, 6, 12, 6 * ALEGO_GRAPH_MAX_LOOPS}) {
    std::vector<double> C((size_t)n * n), Cr;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) C[(size_t)i * n + j] = C[(size_t)j * n + i] = i == j ? n + 1.0 + rnd() : rnd();
    Cr = C;
    ref_serial_chol(&Cr, n);
    for (int lanes : {1, 3, 64}) {
      std::vector<double> Cl = C;
      laned_chol(&Cl, n, lanes);
      if (!same(Cl.data(), Cr.data(), Cl.size())) return fail("pg_chol_dense", n * 100 + lanes);
    }
  }
  // the predicates
  double between[12], var[6];
  for (double bad : {inf, -inf, nan}) {
    for (int k = 0; k < 18; ++k) {
      for (double& x : between) x = 0.25;
      for (double& x : var) x = 0.5;
      (k < 12 ? between[k] : var[k - 12]) = bad;
      if (pg_edge_finite(between, var) || pg_finite(bad)) return fail("pg_edge_finite takes a non-finite number", k);
    }
  }
  for (double& x : between) x = -3.0;
  for (double& x : var) x = 1e-300;
  if (!pg_edge_finite(between, var) || !pg_finite(-1.79769313486231570815e+308)) return fail("pg_edge_finite refuses a finite edge", 0);
  for (double bad : {0.0, -0.0, -1.0}) { var[4] = bad; if (pg_edge_finite(between, var)) return fail("pg_edge_finite takes a variance that is not positive", 0); }
  const int n = 5;
  const int ids[][3] = {{0, 4, 1}, {4, 0, 1}, {-1, 0, 0}, {0, -1, 0}, {n, 0, 0}, {0, n, 0}, {2, 2, 0}, {-1, -1, 0}};
  for (const auto& c : ids) if (pg_loop_ids(c[0], c[1], n) != (c[2] != 0)) return fail("pg_loop_ids", c[0] * 10 + c[1]);
  if (!pg_edge_ids(-1, 0, n, -1) || !pg_edge_ids(-1, 4, n, -1) || pg_edge_ids(-2, 0, n, -1) || pg_edge_ids(-1, -1, n, -1) || pg_edge_ids(-1, n, n, -1) || !pg_edge_ids(3, 1, n, -1) ||
      pg_edge_ids(3, 3, n, -1)) return fail("pg_edge_ids", 0);
  if (!pg_chain_ids(-1, 0, 0) || !pg_chain_ids(2, 3, 3) || pg_chain_ids(0, 0, 0) || pg_chain_ids(1, 3, 3) || pg_chain_ids(2, 3, 2) || pg_chain_ids(3, 2, 3)) return fail("pg_chain_ids", 0);
  g_checks += 3;
  std::fprintf(stderr, "pg_chain ok %d\n", g_checks);
  return true;
}

static bool read_edges(FILE* f, int n, std::vector<alego_graph_edge>* e) {
  e->resize(n);
  for (int i = 0; i < n; ++i) {
    alego_graph_edge& x = (*e)[i];
    if (std::fscanf(f, "%d %d", &x.from, &x.to) != 2) return false;
    for (int k = 0; k < 12; ++k) if (std::fscanf(f, "%la", &x.between[k]) != 1) return false;
    for (int k = 0; k < 6; ++k) if (std::fscanf(f, "%la", &x.variance[k]) != 1) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  if (!chain_checks()) return 1;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  int cases = 0, N, ne, np, nc;
  while (std::fscanf(f, "%d %d %d %d", &N, &ne, &np, &nc) == 4) {
    if (N <= 0 || ne < N || np < 0 || nc < 0) { std::fprintf(stderr, "case %d: bad counts\n", cases); std::fclose(f); return 2; }
    std::vector<double> X((size_t)N * 12);
    for (double& v : X) if (std::fscanf(f, "%la", &v) != 1) { std::fclose(f); return 2; }
    std::vector<alego_graph_edge> edges, cand;
    if (!read_edges(f, ne, &edges)) { std::fclose(f); return 2; }
    std::vector<int> pairs((size_t)np * 2);
    for (int& v : pairs) if (std::fscanf(f, "%d", &v) != 1) { std::fclose(f); return 2; }
    if (!read_edges(f, nc, &cand)) { std::fclose(f); return 2; }
    std::vector<double> marg((size_t)N * 36), pair((size_t)np * 36);
    std::vector<alego_graph_check> out(nc);
    if (pgc_host_covariance(X.data(), N, edges.data(), ne, pairs.data(), np, marg.data(), pair.data()) != 0 ||
        pgc_host_check(X.data(), N, edges.data(), ne, cand.data(), nc, out.data()) != 0) {
      std::fprintf(stderr, "case %d: refused\n", cases); std::fclose(f); return 1;
    }
    std::string line;
    char buf[64];
    auto put = [&](double v) { std::snprintf(buf, sizeof(buf), "%a ", v); line += buf; };
    for (double v : marg) put(v);
    for (double v : pair) put(v);
    for (const alego_graph_check& o : out) {
      put(o.status); put(o.d2);
      for (double v : o.error) put(v);
      for (double v : o.cov) put(v);
    }
    std::puts(line.c_str());
    ++cases;
  }
  std::fclose(f);
  std::printf("pg_cov_math ok %d\n", cases);
  return 0;
}
