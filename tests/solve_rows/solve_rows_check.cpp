// csrc/solve_rows.h on the host: the cost-first trust-region control of lo_solve_t / lm_solve against the evaluation of every point in full.
//  1. eval_block_residual + accumulate_cost against acc[27] of eval_block + accumulate_block, bit for bit, for the four block types over
//     sequences of rows with inliers, outliers of the Huber loss, exactly-zero residuals, and rows with a non-finite residual;
//  2. accumulate_block_cols (the accumulators of a block type's non-zero Jacobian columns, LaserOdometry's surf and corner rows) against
//     accumulate_block, all 28 scalars bit for bit over the same sequences, rows with a non-finite residual or Jacobian (the guard) included;
//  3. whole solves on seeded problems of pipeline-sized geometry: the solver as it was before the split (lm_begin, lm_propose, lm_consume on full
//     evaluations) against lm_control in both candidate policies and in its FULL_EVAL mode — the point, both costs, iterations, successful steps
//     and termination of every outer iteration, bit for bit — with the evaluations counted.
// Built by tests/test_solve_rows.py with -ffp-contract=off and AddressSanitizer + UBSan as a program of its own.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "solve_rows.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() { uint64_t z = (g_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Row { int type; double cp[3], a[3], b[3], c[3], dd; };

static void unit(double v[3]) { const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); for (int k = 0; k < 3; ++k) v[k] /= n; }

// a row whose residual at `truth` is about `off`: the query point is a sensor-frame point (f32, as the device stages it), its geometry sits where
// `truth` puts the point, displaced by `off` across the line / plane
static Row make_row(int type, const double truth[6], double off) {
  Row r{};
  r.type = type;
  for (int k = 0; k < 3; ++k) r.cp[k] = (double)(float)uni(-40.0, 40.0);
  r.cp[2] = (double)(float)uni(-3.0, 6.0);
  const PoseTerms T = pose_terms(truth);
  double lp[3];
  dq_rotate(T.q, r.cp, lp);
  for (int k = 0; k < 3; ++k) lp[k] += T.t[k];
  double n[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)}, u[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
  unit(n);
  const double dot = u[0] * n[0] + u[1] * n[1] + u[2] * n[2];   // u: a direction across n
  for (int k = 0; k < 3; ++k) u[k] -= dot * n[k];
  unit(u);
  double w[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};
  if (type == BLK_PLANE) {   // a = unit normal, dd = -(n . point of the plane)
    for (int k = 0; k < 3; ++k) r.a[k] = n[k];
    r.dd = -(n[0] * lp[0] + n[1] * lp[1] + n[2] * lp[2]) + off;
  } else if (type == BLK_SURF) {   // a, b, c span a plane at distance ~off from the point (the functor's own weighting makes it a residual of that order)
    for (int k = 0; k < 3; ++k) {
      const double base = lp[k] + off * n[k];
      r.a[k] = (double)(float)(base + 0.3 * u[k]); r.b[k] = (double)(float)(base - 0.8 * u[k] + 0.4 * w[k]); r.c[k] = (double)(float)(base - 0.2 * u[k] - 0.9 * w[k]);
    }
  } else {   // a, b on a line along u at distance off from the point
    for (int k = 0; k < 3; ++k) {
      const double base = lp[k] + off * n[k];
      r.a[k] = base + 0.4 * u[k]; r.b[k] = base - 0.7 * u[k];
      if (type == BLK_CORNER) { r.a[k] = (double)(float)r.a[k]; r.b[k] = (double)(float)r.b[k]; }
    }
  }
  return r;
}

static double residual_only(const Row& r, const PoseTerms& T) {
  switch (r.type) {
    case BLK_SURF: return eval_block_residual<BLK_SURF>(r.cp, r.a, r.b, r.c, r.dd, T);
    case BLK_CORNER: return eval_block_residual<BLK_CORNER>(r.cp, r.a, r.b, r.c, r.dd, T);
    case BLK_EDGE: return eval_block_residual<BLK_EDGE>(r.cp, r.a, r.b, r.c, r.dd, T);
    default: return eval_block_residual<BLK_PLANE>(r.cp, r.a, r.b, r.c, r.dd, T);
  }
}

struct Problem {
  std::vector<Row> rows;
  double huber;
  long n_full = 0, n_cost = 0;
  void full(const double* x, double acc[28]) {
    ++n_full;
    for (int k = 0; k < 28; ++k) acc[k] = 0;
    const PoseTerms T = pose_terms(x);
    for (const Row& r : rows) { double res, J[6]; eval_block(r.type, r.cp, r.a, r.b, r.c, r.dd, T, &res, J); accumulate_block(res, J, huber, acc); }
  }
  void cost(const double* x, double acc[28]) {
    ++n_cost;
    for (int k = 0; k < 28; ++k) acc[k] = -7.0;   // (nothing but acc[27] may be read)
    acc[27] = 0;
    const PoseTerms T = pose_terms(x);
    for (const Row& r : rows) accumulate_cost(residual_only(r, T), huber, acc[27]);
  }
};

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

// the solver before the split: every point in full (what lm_solve / lo_solve_body did, what lm_shard_step still does)
static void solve_reference(Problem& P, double* params, int outers, int max_iter, std::vector<Outcome>& out) {
  LmState S;
  double acc[28];
  for (int outer = 0; outer < outers; ++outer) {
    double x0[6];
    for (int k = 0; k < 6; ++k) x0[k] = params[k];
    P.full(x0, acc);
    lm_begin(S, x0, acc, max_iter);
    while (true) {
      const int act = lm_propose(S);
      if (act == LM_STOP) break;
      if (act == LM_EVAL) { P.full(S.cand, acc); if (lm_consume(S, acc) == LM_STOP) break; }
    }
    for (int k = 0; k < 6; ++k) params[k] = S.x[k];
    out.push_back(outcome_of(S));
  }
}

struct Seen { long again = 0, jac = 0, cand_full = 0, cand_cost = 0; };
// the loop of lm_solve_body / lo_solve_body (kernels_lm.hip, kernels_lo.hip)
template <bool FULL_EVAL, bool SPECULATE>
static void solve_split(Problem& P, double* params, int outers, int max_iter, std::vector<Outcome>& out, Seen& seen) {
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
      seen.again += kind == LM_EV_AGAIN; seen.jac += kind == LM_EV_JAC; seen.cand_full += kind == LM_EV_CAND_FULL; seen.cand_cost += kind == LM_EV_CAND_COST;
      const int act = lm_control<FULL_EVAL, SPECULATE>(S, kind, params, acc, max_iter);
      if (act == LM_STOP) break;
      kind = lm_next_eval<FULL_EVAL>(act);
    }
    for (int k = 0; k < 6; ++k) params[k] = S.x[k];
    again = S.jac_valid;
    out.push_back(outcome_of(S));
  }
}

static void check_costs() {
  const double truth[6] = {0.3, -0.2, 0.05, 0.01, -0.02, 0.4};
  const double huber = 0.1;
  for (int type = 0; type < 4; ++type) {
    std::vector<Row> rows;
    for (int i = 0; i < 4000; ++i) {
      const int m = i % 4;   // inlier, outlier of the loss, far outlier, (plane rows: exactly zero at the truth)
      rows.push_back(make_row(type, truth, m == 0 ? uni(-0.05, 0.05) : m == 1 ? uni(0.15, 0.6) : m == 2 ? uni(2.0, 9.0) : 0.0));
    }
    long outl = 0, zero = 0;
    for (int pass = 0; pass < 3; ++pass) {
      double x[6];
      for (int k = 0; k < 6; ++k) x[k] = truth[k] + (pass == 0 ? 0.0 : uni(-0.05, 0.05));
      const PoseTerms T = pose_terms(x);
      for (int stride : {1, 64, 256}) {   // thread t of a workgroup of `stride` sums rows t, t + stride, ...: every partial sum agrees
        for (int t = 0; t < (stride < 8 ? stride : 8); ++t) {
          double acc[28] = {0}, cost = 0;
          for (size_t i = t; i < rows.size(); i += stride) {
            const Row& r = rows[i];
            double res, J[6];
            eval_block(r.type, r.cp, r.a, r.b, r.c, r.dd, T, &res, J);
            accumulate_block(res, J, huber, acc);
            const double res2 = residual_only(r, T);
            CHECK(same_bits(res, res2), "type %d row %zu: residual %.17g != %.17g", type, i, res2, res);
            accumulate_cost(res2, huber, cost);
            CHECK(same_bits(cost, acc[27]), "type %d row %zu stride %d: cost %.17g != %.17g", type, i, stride, cost, acc[27]);
            if (stride == 1 && pass == 0) { outl += res * res > huber * huber; zero += res == 0.0; }
          }
        }
      }
    }
    CHECK(outl > 500 && outl < 3900, "type %d: %ld rows beyond the Huber threshold", type, outl);
    if (type == BLK_PLANE) CHECK(zero > 100, "plane rows with a zero residual: %ld", zero);
    // a non-finite residual: both evaluations deliver a non-finite cost, and the control takes it for the largest double either way
    for (double bad : {(double)INFINITY, (double)NAN}) {
      Row r = rows[0];
      r.cp[1] = bad;
      const PoseTerms T = pose_terms(truth);
      double res, J[6], acc[28] = {0}, cost = 0;
      eval_block(r.type, r.cp, r.a, r.b, r.c, r.dd, T, &res, J);
      accumulate_block(res, J, huber, acc);
      accumulate_cost(residual_only(r, T), huber, cost);
      CHECK(!isfinite(res) && !isfinite(cost) && !isfinite(acc[27]) && (same_bits(cost, acc[27]) || (cost != cost && acc[27] != acc[27])), "type %d: non-finite row: cost %g / %g", type, cost, acc[27]);
    }
  }
}

static bool same_or_both_nan(double a, double b) { return same_bits(a, b) || (a != a && b != b); }

// LaserOdometry's full rows: the specialised accumulators against the generic one
static void check_column_accumulators() {
  const double truth[6] = {0.3, -0.2, 0.05, 0.01, -0.02, 0.4};
  for (int type : {(int)BLK_SURF, (int)BLK_CORNER}) {
    for (double huber : {0.1, 0.01}) {
      std::vector<Row> rows;
      for (int i = 0; i < 4000; ++i) {
        const int m = i % 4;
        rows.push_back(make_row(type, truth, m == 0 ? uni(-0.05, 0.05) : m == 1 ? uni(0.15, 0.6) : m == 2 ? uni(2.0, 9.0) : uni(-0.005, 0.005)));
      }
      // rows the guard has to catch, in mid-sequence: a non-finite query point, and a point exactly on its plane / line (m = 0: residual 0, Jacobian 0 / 0)
      rows[1500].cp[1] = (double)INFINITY;
      rows[2500].cp[0] = (double)NAN;
      const double zero[6] = {0, 0, 0, 0, 0, 0};
      for (int pass = 0; pass < 3; ++pass) {
        double x[6];
        for (int k = 0; k < 6; ++k) x[k] = pass == 2 ? zero[k] : truth[k] + (pass == 0 ? 0.0 : uni(-0.05, 0.05));
        if (pass == 2) { Row& r = rows[700]; for (int k = 0; k < 3; ++k) r.cp[k] = r.a[k]; }   // pose zero: lp = cp = a exactly
        const PoseTerms T = pose_terms(x);
        double gen[28] = {0}, spec[28] = {0};
        long guarded = 0;
        for (size_t i = 0; i < rows.size(); ++i) {
          const Row& r = rows[i];
          double res, J[6];
          eval_block(r.type, r.cp, r.a, r.b, r.c, r.dd, T, &res, J);
          for (int k = 0; k < 6; ++k) if (!(((type == BLK_SURF ? (int)COLS_SURF : (int)COLS_CORNER) >> k) & 1)) CHECK(same_bits(J[k], 0.0), "type %d: column %d is not a hard zero", type, k);
          bool fin = isfinite(res);
          for (int k = 0; k < 6; ++k) fin = fin && isfinite(J[k]);
          guarded += !fin;
          accumulate_block(res, J, huber, gen);
          if (type == BLK_SURF) accumulate_block_cols<COLS_SURF>(res, J, huber, spec); else accumulate_block_cols<COLS_CORNER>(res, J, huber, spec);
          if (i == 1499 || i == rows.size() - 1)   // before the first guarded row (row 700 joins them in the last pass, and stays): every scalar finite and equal; afterwards: NaNs in the same places
            for (int k = 0; k < 28; ++k) CHECK((i == 1499 && pass < 2) ? same_bits(gen[k], spec[k]) && isfinite(gen[k]) : same_or_both_nan(gen[k], spec[k]), "type %d huber %g pass %d row %zu: acc[%d] %.17g != %.17g", type, huber, pass, i, k, spec[k], gen[k]);
        }
        CHECK(guarded >= (pass == 2 ? 3 : 2), "type %d pass %d: %ld rows for the guard", type, pass, guarded);
      }
    }
  }
  // a sequence without non-finite rows, summed to the end: bit for bit
  for (int type : {(int)BLK_SURF, (int)BLK_CORNER}) {
    const PoseTerms T = pose_terms(truth);
    double gen[28] = {0}, spec[28] = {0};
    for (int i = 0; i < 3000; ++i) {
      const Row r = make_row(type, truth, i % 3 == 0 ? uni(-0.05, 0.05) : uni(-1.0, 1.0));
      double res, J[6];
      eval_block(r.type, r.cp, r.a, r.b, r.c, r.dd, T, &res, J);
      accumulate_block(res, J, 0.1, gen);
      if (type == BLK_SURF) accumulate_block_cols<COLS_SURF>(res, J, 0.1, spec); else accumulate_block_cols<COLS_CORNER>(res, J, 0.1, spec);
    }
    for (int k = 0; k < 28; ++k) CHECK(same_bits(gen[k], spec[k]) && isfinite(gen[k]), "type %d: acc[%d] %.17g != %.17g", type, k, spec[k], gen[k]);
    CHECK(gen[tri(2, 2)] > 0 || type == BLK_CORNER, "surf rows left J^T J (2, 2) at %g", gen[tri(2, 2)]);
  }
}

static void check_solves() {
  long n_acc = 0, n_rej = 0, term[6] = {0}, ref_full = 0, lazy_full[2] = {0}, lazy_cost[2] = {0};
  Seen seen[2];
  for (int prob = 0; prob < 240; ++prob) {
    const bool odometry = prob & 1;   // surf + corner rows (LaserOdometry) | edge + plane rows (LaserMapping)
    const int max_iter = (const int[]){1, 2, 5, 20, 0, 3}[prob % 6];
    const int outers = odometry ? 1 : 2 + (prob % 3 == 0);
    Problem P;
    P.huber = (prob % 5 == 0) ? 0.01 : 0.1;
    const double truth[6] = {uni(-0.5, 0.5), uni(-0.5, 0.5), uni(-0.1, 0.1), uni(-0.03, 0.03), uni(-0.03, 0.03), uni(-0.3, 0.3)};
    const int n0 = odometry ? 300 : 250, n1 = odometry ? 150 : 650;
    const double noise = (prob % 4 == 0) ? 0.3 : 0.03;
    for (int i = 0; i < n0; ++i) P.rows.push_back(make_row(odometry ? BLK_SURF : BLK_EDGE, truth, (i % 7 == 0 ? 1.5 : noise) * uni(-1, 1)));
    for (int i = 0; i < n1; ++i) P.rows.push_back(make_row(odometry ? BLK_CORNER : BLK_PLANE, truth, (i % 9 == 0 ? 1.5 : noise) * uni(-1, 1)));
    double start[6];
    const double far = (prob % 3 == 1) ? 6.0 : 1.0;
    for (int k = 0; k < 6; ++k) start[k] = truth[k] + far * (k < 3 ? uni(-0.3, 0.3) : uni(-0.05, 0.05));
    if (prob == 17) P.rows[3].cp[0] = NAN;   // a non-finite cost at the start: termination 4 on every path
    if (prob == 23) P.rows.clear();          // (the kernels never solve an empty problem; the control must still agree)
    std::vector<Outcome> ref, a, b, c;
    double pr[6], pa[6], pb[6], pc[6];
    for (int k = 0; k < 6; ++k) pr[k] = pa[k] = pb[k] = pc[k] = start[k];
    solve_reference(P, pr, outers, max_iter, ref);
    ref_full += P.n_full; P.n_full = P.n_cost = 0;
    solve_split<false, false>(P, pa, outers, max_iter, a, seen[0]);
    lazy_full[0] += P.n_full; lazy_cost[0] += P.n_cost; P.n_full = P.n_cost = 0;
    solve_split<false, true>(P, pb, outers, max_iter, b, seen[1]);
    lazy_full[1] += P.n_full; lazy_cost[1] += P.n_cost; P.n_full = P.n_cost = 0;
    Seen unused;
    solve_split<true, false>(P, pc, outers, max_iter, c, unused);
    CHECK(P.n_cost == 0 && unused.again == 0 && unused.jac == 0 && unused.cand_cost == 0, "problem %d: the FULL_EVAL control left the full path", prob);
    for (int o = 0; o < outers; ++o) {
      CHECK(same_outcome(ref[o], a[o]), "problem %d outer %d cost-first: iter %d/%d succ %d/%d term %d/%d cost %.17g/%.17g", prob, o, a[o].iter, ref[o].iter, a[o].successful, ref[o].successful, a[o].termination, ref[o].termination, a[o].x_cost, ref[o].x_cost);
      CHECK(same_outcome(ref[o], b[o]), "problem %d outer %d speculative: iter %d/%d succ %d/%d term %d/%d", prob, o, b[o].iter, ref[o].iter, b[o].successful, ref[o].successful, b[o].termination, ref[o].termination);
      CHECK(same_outcome(ref[o], c[o]), "problem %d outer %d FULL_EVAL: iter %d/%d", prob, o, c[o].iter, ref[o].iter);
      n_acc += ref[o].successful;
      n_rej += ref[o].iter - ref[o].successful - (ref[o].termination == 2 || ref[o].termination == 3);
      ++term[ref[o].termination];
    }
  }
  std::printf("solves: accepted %ld rejected %ld terminations [limit %ld, gradient %ld, step %ld, cost %ld, failure %ld, radius %ld]\n", n_acc, n_rej, term[0], term[1], term[2], term[3], term[4], term[5]);
  std::printf("evaluations: reference %ld full | cost-first %ld full + %ld cost (begin-again %ld, lazy Jacobians %ld) | speculative %ld full + %ld cost (begin-again %ld, lazy %ld, candidates in full %ld)\n",
              ref_full, lazy_full[0], lazy_cost[0], seen[0].again, seen[0].jac, lazy_full[1], lazy_cost[1], seen[1].again, seen[1].jac, seen[1].cand_full);
  // the premise: these problems drive every path of the control
  CHECK(n_acc > 100 && n_rej > 20, "accepted %ld rejected %ld", n_acc, n_rej);
  CHECK(term[0] > 20 && term[3] > 20 && term[4] >= 1, "terminations %ld %ld %ld", term[0], term[3], term[4]);
  CHECK(seen[0].again > 10 && seen[0].jac > 50 && seen[0].cand_full == 0, "cost-first paths: %ld %ld %ld", seen[0].again, seen[0].jac, seen[0].cand_full);
  CHECK(seen[1].again > 10 && seen[1].jac > 5 && seen[1].cand_full > 50 && seen[1].cand_cost > 20, "speculative paths: %ld %ld %ld %ld", seen[1].again, seen[1].jac, seen[1].cand_full, seen[1].cand_cost);
  // a point is evaluated once for its cost and at most once more in full: never more passes than candidates + points
  CHECK(lazy_full[0] < ref_full && lazy_full[1] < ref_full && lazy_full[0] <= lazy_full[1], "full evaluations %ld / %ld against %ld", lazy_full[0], lazy_full[1], ref_full);
}

int main() {
  check_costs();
  check_column_accumulators();
  check_solves();
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("solve_rows ok\n");
  return 0;
}
