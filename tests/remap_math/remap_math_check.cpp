// csrc/remap_math.h and the projected lm_step of csrc/solve_rows.h on the host:
//  1. the projector of constructed problems: P P = P and Pt v_held = 0 at rounding level, P the exact identity when nothing is held and exactly zero
//     when everything is, every status, and nothing held with a status other than 1;
//  2. lm_step<true> with proj = null against lm_step<false>, bit for bit, over many states;
//  3. whole solves under the projection: the solver that evaluates every point in full against lm_control in both candidate policies and in its
//     FULL_EVAL mode, bit for bit, and the shift M0 (x_final - x0) . v_held of every held direction of every problem;
//  4. the front remap_math.h shares with reg_cov_math.h (rc_spectrum): rc_compute and rm_compute on the same inputs at the guards' edges and at
//     repeated eigenvalues — equal statuses, the same bits in eigval and eigvec, n_degenerate == n_held.
// Built by tests/test_remap_math.py with -ffp-contract=off and AddressSanitizer + UBSan as a program of its own.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "solve_rows.h"

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64() { uint64_t z = (g_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Row { int type; double cp[3], a[3], b[3], dd; };
struct Problem {
  std::vector<Row> rows;
  double huber = 0.1;
  void full(const double* x, double acc[28]) const {
    for (int k = 0; k < 28; ++k) acc[k] = 0;
    const PoseTerms T = pose_terms(x);
    const double c3[3] = {0, 0, 0};
    for (const Row& r : rows) { double res, J[6]; eval_block(r.type, r.cp, r.a, r.b, c3, r.dd, T, &res, J); accumulate_block(res, J, huber, acc); }
  }
  void cost(const double* x, double acc[28]) const {
    for (int k = 0; k < 28; ++k) acc[k] = -7.0;
    acc[27] = 0;
    const PoseTerms T = pose_terms(x);
    const double c3[3] = {0, 0, 0};
    for (const Row& r : rows)
      accumulate_cost(r.type == BLK_EDGE ? eval_block_residual<BLK_EDGE>(r.cp, r.a, r.b, c3, r.dd, T) : eval_block_residual<BLK_PLANE>(r.cp, r.a, r.b, c3, r.dd, T), huber, acc[27]);
  }
};

// world point -> sensor-frame query (f32, as the device keeps it) at pose p
static void to_sensor(const double p[6], const double w[3], double out[3]) {
  const PoseTerms T = pose_terms(p);
  const DQuat qi{T.q.w, -T.q.x, -T.q.y, -T.q.z};
  const double d[3] = {w[0] - p[0], w[1] - p[1], w[2] - p[2]};
  dq_rotate(qi, d, out);
  for (int k = 0; k < 3; ++k) out[k] = (double)(float)out[k];
}
static Row plane_row(const double p[6], const double n[3], const double on[3], double off) {
  Row r{};
  r.type = BLK_PLANE;
  const double w[3] = {on[0] + off * n[0], on[1] + off * n[1], on[2] + off * n[2]};
  to_sensor(p, w, r.cp);
  for (int k = 0; k < 3; ++k) r.a[k] = n[k];
  r.dd = -(n[0] * on[0] + n[1] * on[1] + n[2] * on[2]);
  return r;
}
static Row edge_row(const double p[6], const double on[3], const double dir[3], const double off[3]) {
  Row r{};
  r.type = BLK_EDGE;
  const double w[3] = {on[0] + off[0], on[1] + off[1], on[2] + off[2]};
  to_sensor(p, w, r.cp);
  for (int k = 0; k < 3; ++k) { r.a[k] = on[k] + 0.1 * dir[k]; r.b[k] = on[k] - 0.1 * dir[k]; }
  return r;
}
// kind 0: a corridor along x (nothing observes translation x) with `spur` wrong rows of a wall across it; 1: a floor alone (x, y and yaw free);
// 2: walls, floor and lines along every axis (nothing held at eig_min 10)
static Problem make_problem(int kind, const double truth[6], int spur) {
  Problem P;
  const double ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0}, ez[3] = {0, 0, 1}, eyn[3] = {0, -1, 0};
  for (int i = 0; i < 120; ++i) {
    const double big = i % 9 == 0 ? 0.3 : 0.01;
    const double f[3] = {uni(-6, 6), uni(-2, 2), -1.3}, l[3] = {uni(-6, 6), 2.0, uni(-1, 2)}, r[3] = {uni(-6, 6), -2.0, uni(-1, 2)};
    P.rows.push_back(plane_row(truth, ez, f, big * uni(-1, 1)));
    if (kind != 1) { P.rows.push_back(plane_row(truth, ey, l, big * uni(-1, 1))); P.rows.push_back(plane_row(truth, eyn, r, big * uni(-1, 1))); }
    if (kind == 2) { const double w[3] = {9.0, uni(-2, 2), uni(-1, 2)}; P.rows.push_back(plane_row(truth, ex, w, big * uni(-1, 1))); }
  }
  if (kind != 1)
    for (int i = 0; i < 40; ++i) {
      const double on[3] = {uni(-6, 6), i % 2 ? 1.9 : -1.9, 2.2}, off[3] = {0, 0.01 * uni(-1, 1), 0.01 * uni(-1, 1)};
      P.rows.push_back(edge_row(truth, on, ex, off));
      if (kind == 2) { const double o2[3] = {6, 4, uni(-1, 2)}, f2[3] = {0.01 * uni(-1, 1), 0.01 * uni(-1, 1), 0}; P.rows.push_back(edge_row(truth, o2, ez, f2)); }
    }
  for (int i = 0; i < spur; ++i) { const double w[3] = {8.0, uni(-1.5, 1.5), uni(-1, 2)}; P.rows.push_back(plane_row(truth, ex, w, 0.4)); }
  return P;
}

struct Outcome { double x[6], initial_cost, x_cost; int iter, successful, termination; };
static Outcome outcome_of(const LmState& S) {
  Outcome o;
  for (int k = 0; k < 6; ++k) o.x[k] = S.x[k];
  o.initial_cost = S.initial_cost; o.x_cost = S.x_cost; o.iter = S.iter; o.successful = S.successful; o.termination = S.termination;
  return o;
}
static bool same_outcome(const Outcome& a, const Outcome& b) {
  for (int k = 0; k < 6; ++k) if (!same_bits(a.x[k], b.x[k])) return false;
  return same_bits(a.initial_cost, b.initial_cost) && same_bits(a.x_cost, b.x_cost) && a.iter == b.iter && a.successful == b.successful && a.termination == b.termination;
}
// every point in full, the projection in every step
static void solve_reference(const Problem& P, double* params, int outers, int max_iter, const double* proj, std::vector<Outcome>& out) {
  LmState S;
  double acc[28];
  for (int outer = 0; outer < outers; ++outer) {
    double x0[6];
    for (int k = 0; k < 6; ++k) x0[k] = params[k];
    P.full(x0, acc);
    lm_begin(S, x0, acc, max_iter);
    while (true) {
      const int act = lm_propose<true>(S, proj);
      if (act == LM_STOP) break;
      if (act == LM_EVAL) { P.full(S.cand, acc); if (lm_consume(S, acc) == LM_STOP) break; }
    }
    for (int k = 0; k < 6; ++k) params[k] = S.x[k];
    out.push_back(outcome_of(S));
  }
}
// the loop of lm_solve_body
template <bool FULL_EVAL, bool SPECULATE>
static void solve_split(const Problem& P, double* params, int outers, int max_iter, const double* proj, std::vector<Outcome>& out) {
  LmState S;
  std::memset(&S, 0xA5, sizeof S);
  double acc[28];
  int again = 0;
  for (int outer = 0; outer < outers; ++outer) {
    int kind = (!FULL_EVAL && outer > 0 && again) ? LM_EV_AGAIN : LM_EV_BEGIN;
    while (true) {
      double x[6];
      for (int k = 0; k < 6; ++k) x[k] = kind == LM_EV_BEGIN ? params[k] : kind == LM_EV_JAC ? S.x[k] : kind == LM_EV_AGAIN ? 0.0 : S.cand[k];
      if (kind == LM_EV_CAND_COST) P.cost(x, acc);
      else if (kind != LM_EV_AGAIN) P.full(x, acc);
      const int act = lm_control<FULL_EVAL, SPECULATE, true>(S, kind, params, acc, max_iter, proj);
      if (act == LM_STOP) break;
      kind = lm_next_eval<FULL_EVAL>(act);
    }
    for (int k = 0; k < 6; ++k) params[k] = S.x[k];
    again = S.jac_valid;
    out.push_back(outcome_of(S));
  }
}

static double max_abs(const double* a, int n) { double m = 0; for (int k = 0; k < n; ++k) m = fmax(m, fabs(a[k])); return m; }

static void check_projector_and_solves() {
  double worst_pp = 0, worst_ptv = 0, worst_shift = 0;
  long held_hist[7] = {0}, term[6] = {0};
  for (int prob = 0; prob < 60; ++prob) {
    const int kind = prob % 3, spur = kind == 0 ? (prob % 4) * 3 : 0;
    const double eig_min = prob % 10 == 9 ? 1e30 : (prob % 10 == 8 ? 1e-300 : kind == 2 ? 10.0 : 100.0);
    const double truth[6] = {uni(-3, 3), uni(-0.3, 0.3), uni(-0.1, 0.1), uni(-0.3, 0.3), prob % 7 == 0 ? -1.0 : uni(-0.3, 0.3), uni(-3, 3)};
    const Problem P = make_problem(kind, truth, spur);
    double start[6];
    for (int k = 0; k < 6; ++k) start[k] = truth[k] + (k < 3 ? uni(-0.15, 0.15) : uni(-0.015, 0.015));
    double acc[28], lam[6], V[36], Pm[36];
    int held = -1;
    P.full(start, acc);
    const int st = rm_compute(acc, start, (int)P.rows.size(), 0, eig_min, lam, V, Pm, &held);
    CHECK(st == 1, "problem %d: status %d", prob, st);
    // the premise: the corridor does not observe translation along it, the floor alone neither x, y nor yaw, the courtyard everything
    if (eig_min == 100.0) CHECK(kind == 0 ? (held >= 1 && lam[0] < 10.0) : (held >= 3 && lam[2] < 1e-6), "problem %d kind %d: %d held (%.3g %.3g %.3g %.3g)", prob, kind, held, lam[0], lam[1], lam[2], lam[3]);
    if (eig_min == 10.0) CHECK(held == 0, "problem %d kind %d: %d held (%.3g)", prob, kind, held, lam[0]);
    if (eig_min == 1e30) CHECK(held == 6, "problem %d: %d held", prob, held);
    { int n = 0; for (int k = 0; k < 6; ++k) n += lam[k] < eig_min; CHECK(n == held, "problem %d: %d held, %d eigenvalues below eig_min", prob, held, n); }
    ++held_hist[held];
    double M[36], N[36];
    rc_m(start, M); rc_minv(start, N);
    if (held == 0) for (int k = 0; k < 36; ++k) CHECK(same_bits(Pm[k], k % 7 == 0 ? 1.0 : 0.0), "problem %d: P[%d] = %.17g with nothing held", prob, k, Pm[k]);
    if (held == 6) for (int k = 0; k < 36; ++k) CHECK(same_bits(Pm[k], 0.0), "problem %d: P[%d] = %.17g with everything held", prob, k, Pm[k]);
    // P P - P, and Pt v_held with Pt = M P N
    double PP[36], MP[36], Pt[36];
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) { double s = 0, t = 0; for (int k = 0; k < 6; ++k) { s += Pm[i * 6 + k] * Pm[k * 6 + j]; t += M[i * 6 + k] * Pm[k * 6 + j]; } PP[i * 6 + j] = s - Pm[i * 6 + j]; MP[i * 6 + j] = t; }
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) { double s = 0; for (int k = 0; k < 6; ++k) s += MP[i * 6 + k] * N[k * 6 + j]; Pt[i * 6 + j] = s; }
    const double scaleP = fmax(1.0, max_abs(Pm, 36));
    worst_pp = fmax(worst_pp, max_abs(PP, 36) / (scaleP * scaleP));
    for (int h = 0; h < held && held < 6; ++h) for (int i = 0; i < 6; ++i) { double s = 0; for (int k = 0; k < 6; ++k) s += Pt[i * 6 + k] * V[k * 6 + h]; worst_ptv = fmax(worst_ptv, fabs(s) / scaleP); }
    // whole solves
    const double* proj = (held > 0) ? Pm : nullptr;
    const int max_iter = (const int[]){10, 2, 5, 20, 1, 3}[prob % 6], outers = 2 + (prob % 5 == 0);
    std::vector<Outcome> ref, a, b, c;
    double pr[6], pa[6], pb[6], pc[6];
    for (int k = 0; k < 6; ++k) pr[k] = pa[k] = pb[k] = pc[k] = start[k];
    solve_reference(P, pr, outers, max_iter, proj, ref);
    solve_split<false, false>(P, pa, outers, max_iter, proj, a);
    solve_split<false, true>(P, pb, outers, max_iter, proj, b);
    solve_split<true, false>(P, pc, outers, max_iter, proj, c);
    for (int o = 0; o < outers; ++o) {
      CHECK(same_outcome(ref[o], a[o]), "problem %d outer %d cost-first: iter %d/%d term %d/%d", prob, o, a[o].iter, ref[o].iter, a[o].termination, ref[o].termination);
      CHECK(same_outcome(ref[o], b[o]), "problem %d outer %d speculative: iter %d/%d term %d/%d", prob, o, b[o].iter, ref[o].iter, b[o].termination, ref[o].termination);
      CHECK(same_outcome(ref[o], c[o]), "problem %d outer %d FULL_EVAL: iter %d/%d", prob, o, c[o].iter, ref[o].iter);
      ++term[ref[o].termination];
    }
    if (held == 6) {
      for (int o = 0; o < outers; ++o) { CHECK(ref[o].termination == 2 && ref[o].iter == 1, "problem %d: everything held ends with %d after %d", prob, ref[o].termination, ref[o].iter); for (int k = 0; k < 6; ++k) CHECK(same_bits(ref[o].x[k], start[k]), "problem %d: moved", prob); }
    }
    // M0 (x_final - x0) . v_held
    double dx[6], xi[6];
    for (int k = 0; k < 6; ++k) dx[k] = pr[k] - start[k];
    for (int i = 0; i < 6; ++i) { double s = 0; for (int k = 0; k < 6; ++k) s += M[i * 6 + k] * dx[k]; xi[i] = s; }
    for (int h = 0; h < held; ++h) { double s = 0; for (int k = 0; k < 6; ++k) s += V[k * 6 + h] * xi[k]; worst_shift = fmax(worst_shift, fabs(s)); }
    if (kind == 0 && spur >= 6 && eig_min == 100.0) {   // the premise: without the projection these rows drag the pose along the corridor
      std::vector<Outcome> plain;
      double pp[6];
      for (int k = 0; k < 6; ++k) pp[k] = start[k];
      solve_reference(P, pp, outers, 10, nullptr, plain);
      double s = 0;
      for (int i = 0; i < 6; ++i) { double t = 0; for (int k = 0; k < 6; ++k) t += M[i * 6 + k] * (pp[k] - start[k]); s += V[i * 6 + 0] * t; }
      CHECK(fabs(s) > 0.1, "problem %d: the plain solver moved %.3g along the held direction", prob, s);
    }
  }
  std::printf("projector: |P P - P| %.3g  |Pt v_held| %.3g  largest |M0 (x_final - x0) . v_held| %.3g\n", worst_pp, worst_ptv, worst_shift);
  std::printf("held counts [%ld %ld %ld %ld %ld %ld %ld]  terminations [%ld %ld %ld %ld %ld %ld]\n", held_hist[0], held_hist[1], held_hist[2], held_hist[3], held_hist[4], held_hist[5],
              held_hist[6], term[0], term[1], term[2], term[3], term[4], term[5]);
  CHECK(worst_pp < 1e-12 && worst_ptv < 1e-12, "projector residuals %.3g %.3g", worst_pp, worst_ptv);
  CHECK(worst_shift < 1e-12, "shift along a held direction %.3g", worst_shift);
  CHECK(held_hist[0] >= 10 && held_hist[1] + held_hist[2] >= 10 && held_hist[3] + held_hist[4] >= 10 && held_hist[6] >= 5, "held counts");
  CHECK(term[0] >= 5 && term[2] >= 10 && term[3] >= 10, "terminations");
}

static void check_statuses() {
  const double truth[6] = {0.3, -0.2, 0.05, 0.01, -0.02, 0.4};
  const Problem P = make_problem(2, truth, 0);
  double acc[28], lam[6], V[36], Pm[36];
  int held = -1;
  P.full(truth, acc);
  auto empty = [&]() { bool z = held == 0; for (int k = 0; k < 36; ++k) z = z && V[k] == 0.0 && Pm[k] == 0.0; for (int k = 0; k < 6; ++k) z = z && lam[k] == 0.0; return z; };
  CHECK(rm_compute(acc, truth, 3, 3, 100.0, lam, V, Pm, &held) == 0 && empty(), "six rows");
  CHECK(rm_compute(acc, truth, 4, 3, 100.0, lam, V, Pm, &held) == 1 && held == 0, "seven rows");
  double up[6];
  for (int k = 0; k < 6; ++k) up[k] = truth[k];
  up[4] = 1.5707963267948966;
  CHECK(rm_compute(acc, up, 100, 100, 100.0, lam, V, Pm, &held) == -3 && empty(), "pitch pi / 2");
  double bad[28];
  for (int k = 0; k < 28; ++k) bad[k] = acc[k];
  bad[5] = NAN;
  CHECK(rm_compute(bad, truth, 100, 100, 100.0, lam, V, Pm, &held) == -2 && empty(), "NaN in the sums");
  bad[5] = acc[5]; bad[27] = INFINITY;
  CHECK(rm_compute(bad, truth, 100, 100, 100.0, lam, V, Pm, &held) == -2 && empty(), "infinite cost");
  for (int k = 0; k < 6; ++k) up[k] = truth[k];
  up[0] = INFINITY;
  CHECK(rm_compute(acc, up, 100, 100, 100.0, lam, V, Pm, &held) == -2 && empty(), "infinite start");
  double e = 0, raw = -1.0;
  CHECK(rm_resolve(nullptr, &e) == 0 && e == RC_DEFAULT_EIG_MIN, "default");
  CHECK(rm_resolve(&raw, &e) == 0 && e == RC_DEFAULT_EIG_MIN, "<= 0");
  raw = 7.5;
  CHECK(rm_resolve(&raw, &e) == 0 && e == 7.5, "given");
  raw = NAN;
  CHECK(rm_resolve(&raw, &e) == -1, "NaN");
  raw = INFINITY;
  CHECK(rm_resolve(&raw, &e) == -1, "inf");
}

// lm_step<true> with no projector is lm_step<false>
static void check_plain_step() {
  for (int t = 0; t < 400; ++t) {
    double J[40][6], r[40], acc[28] = {0};
    for (int i = 0; i < 40; ++i) { for (int k = 0; k < 6; ++k) J[i][k] = (t % 5 == 0 && k == 0) ? 0.0 : uni(-1, 1) * (k < 3 ? 1.0 : 8.0); r[i] = uni(-0.3, 0.3); accumulate_block(r[i], J[i], 0.1, acc); }
    double x0[6];
    for (int k = 0; k < 6; ++k) x0[k] = uni(-1, 1);
    LmState A, B;
    std::memset(&A, 0, sizeof A);
    lm_begin(A, x0, acc, 10);
    A.radius = (const double[]){1e4, 1.0, 1e-3, 1e-20}[t % 4];
    std::memcpy(&B, &A, sizeof A);
    const int ra = lm_step<false>(A), rb = lm_step<true>(B, nullptr);
    CHECK(ra == rb && std::memcmp(&A, &B, sizeof A) == 0, "state %d: lm_step<true>(null) differs (%d / %d)", t, ra, rb);
  }
}

// rc_compute and rm_compute are two tails of one front (rc_spectrum, reg_cov_math.h): on the same (acc28, p, counts) and the same eig_min the statuses
// are equal, eigval and eigvec are the same bits and n_degenerate == n_held — at the guards' edges, where a copy of the front could drift from the other
static int g_front_cases = 0;
static void same_front(const char* what, const double* acc, const double* p, int n_edge, int n_plane, double eig_min, int want_status) {
  const double var_min[6] = {1e-12, 1e-12, 1e-12, 1e-12, 1e-12, 1e-12};
  double opt[RC_OPT_W], s2, info[36], lc[6], Vc[36], cov[36], var[6], lm[6], Vm[36], Pm[36];
  int ndeg = -1, held = -2, sweeps = -1;
  CHECK(rc_resolve(nullptr, var_min, opt) == 0, "%s: options", what);
  opt[RC_EIG_MIN] = eig_min;
  const int sc = rc_compute(acc, p, n_edge, n_plane, opt, &s2, info, lc, Vc, cov, var, &ndeg, &sweeps);
  const int sm = rm_compute(acc, p, n_edge, n_plane, eig_min, lm, Vm, Pm, &held);
  CHECK(sc == sm && sc == want_status, "%s: status %d (regcov) %d (remap), expected %d", what, sc, sm, want_status);
  CHECK(ndeg == held, "%s: n_degenerate %d, n_held %d", what, ndeg, held);
  for (int k = 0; k < 6; ++k) CHECK(same_bits(lc[k], lm[k]), "%s: eigval[%d] %.17g / %.17g", what, k, lc[k], lm[k]);
  for (int k = 0; k < 36; ++k) CHECK(same_bits(Vc[k], Vm[k]), "%s: eigvec[%d] %.17g / %.17g", what, k, Vc[k], Vm[k]);
  if (sc == 1) { int n = 0; for (int k = 0; k < 6; ++k) n += lc[k] < eig_min; CHECK(n == held, "%s: %d eigenvalues below eig_min, %d held", what, n, held); }
  ++g_front_cases;
}
static void check_shared_front() {
  const double truth[6] = {0.3, -0.2, 0.05, 0.01, -0.02, 0.4};
  const Problem well = make_problem(2, truth, 0), corridor = make_problem(0, truth, 6);
  double acc[28], cor[28];
  well.full(truth, acc);
  corridor.full(truth, cor);
  // the fixtures of this program: everything observed; a corridor that does not observe translation along it
  same_front("courtyard", acc, truth, 40 * 2, 120 * 4, 10.0, 1);
  same_front("corridor", cor, truth, 40, 120 * 3 + 6, 100.0, 1);
  { double lam[6], V[36], Pm[36]; int held = 0; CHECK(rm_compute(cor, truth, 40, 366, 100.0, lam, V, Pm, &held) == 1 && held >= 1, "the corridor holds %d", held); }
  // the row-count edge
  same_front("six rows", acc, truth, 3, 3, 10.0, 0);
  same_front("seven rows", acc, truth, 3, 4, 10.0, 1);
  // the two neighbouring pitches whose |cos| straddle RC_COS_PITCH_MIN (cos moves by about one ulp of the pitch per ulp of the pitch there: no
  // double has a cosine closer to the bound on either side)
  double below[6], above[6];
  for (int k = 0; k < 6; ++k) below[k] = above[k] = truth[k];
  double a = acos(RC_COS_PITCH_MIN);
  while (fabs(cos(a)) < RC_COS_PITCH_MIN) a = nextafter(a, 0.0);
  while (!(fabs(cos(a)) < RC_COS_PITCH_MIN)) a = nextafter(a, 2.0);   // a: the first pitch past the bound
  below[4] = a; above[4] = nextafter(a, 0.0);
  CHECK(fabs(cos(below[4])) < RC_COS_PITCH_MIN && !(fabs(cos(above[4])) < RC_COS_PITCH_MIN), "pitches %.17g %.17g do not straddle the bound", below[4], above[4]);
  same_front("|cos pitch| just below the bound", acc, below, 100, 100, 10.0, -3);
  same_front("|cos pitch| just at or above the bound", acc, above, 100, 100, 10.0, 1);
  below[4] = -below[4]; above[4] = -above[4];
  same_front("|cos pitch| just below the bound, pitch < 0", acc, below, 100, 100, 10.0, -3);
  same_front("|cos pitch| just at or above the bound, pitch < 0", acc, above, 100, 100, 10.0, 1);
  // a NaN and an infinity in the sums and in the pose (the row and pitch guards come first: six rows with a NaN is status 0, pitch NaN is -2)
  for (int where = 0; where < 4; ++where)
    for (int inf = 0; inf < 2; ++inf) {
      double b[28], q[6];
      for (int k = 0; k < 28; ++k) b[k] = acc[k];
      for (int k = 0; k < 6; ++k) q[k] = truth[k];
      const double v = inf ? (where % 2 ? -INFINITY : INFINITY) : NAN;
      if (where == 0) b[7] = v; else if (where == 1) b[27] = v; else if (where == 2) q[1] = v; else q[4] = v;
      same_front(inf ? "an infinity" : "a NaN", b, q, 100, 100, 10.0, -2);
      if (where == 0) same_front("six rows and a value that is not finite", b, q, 6, 0, 10.0, 0);
    }
  // repeated eigenvalues, p = 0 (N is a permutation: info is H with its halves exchanged): a diagonal H, where the Jacobi makes no rotation and
  // the order is the tie rule's alone, and 4 I + u u^T, whose eigenvalue 4 has multiplicity five; eig_min between, at, and beside the values
  const double zero[6] = {0, 0, 0, 0, 0, 0}, u[6] = {1, -2, 0.5, 3, -1, 2};
  double diag[28] = {0}, rank1[28] = {0};
  const double d[6] = {5, 2, 5, 2, 9, 2};
  for (int i = 0, k = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) { diag[k] = i == j ? d[i] : 0.0; rank1[k] = (i == j ? 4.0 : 0.0) + u[i] * u[j]; }
  diag[27] = rank1[27] = 0.5;
  for (double eig_min : {1.0, 2.0, 3.0, 5.0, 7.0, 100.0}) { same_front("a diagonal H with ties", diag, zero, 50, 50, eig_min, 1); same_front("4 I + u u^T", rank1, zero, 50, 50, eig_min, 1); }
  {
    double lam[6], V[36], Pm[36];
    int held = 0;
    CHECK(rm_compute(diag, zero, 50, 50, 3.0, lam, V, Pm, &held) == 1 && held == 3, "diagonal ties: %d held", held);
    const double want[6] = {2, 2, 2, 5, 5, 9};
    const int col[6] = {0, 2, 4, 3, 5, 1};   // info = diag(2, 9, 2, 5, 2, 5): ascending, ties by index
    for (int k = 0; k < 6; ++k) { CHECK(same_bits(lam[k], want[k]), "diagonal ties: eigval[%d] %.17g", k, lam[k]); for (int i = 0; i < 6; ++i) CHECK(same_bits(V[i * 6 + k], i == col[k] ? 1.0 : 0.0), "diagonal ties: eigvec(%d, %d) %.17g", i, k, V[i * 6 + k]); }
  }
  std::printf("shared front: %d inputs through rc_compute and rm_compute\n", g_front_cases);
}

int main() {
  check_statuses();
  check_shared_front();
  check_plain_step();
  check_projector_and_solves();
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("remap_math ok\n");
  return 0;
}
