// csrc/lm_rows.h on the host: what a registration row of LaserMapping is, held to the layout as this file states it with literal indices.
//  1. layout: rows go through the writers (lmb_put_edge / lmb_put_plane / lmb_put_none, lms_put, lml_put_edge / lml_put_plane) and come back
//     through each of the three readers (block + point, streamed record, LDS arrays), every field bit-equal to the input and to
//     block [0..2] a | normal, [3..5] b, [6] d, [7] type; streamed record [0..7] the block, float4 at double 8;
//  2. split: lml_split / lml_offsets against Ce = min(Rc, budget / 60), Cp = min(Rs, (budget - 60 Ce) / 44) at the budgets where they have edges;
//  3. evaluators: lm_eval_edge / lm_eval_plane, full and cost-only, against eval_block + accumulate_block / eval_block_residual + accumulate_cost
//     called with a zero third point as lm_solve's row loop calls them, bit for bit, residuals on both sides of the Huber delta, a plane with d = 0;
//  4. guard: each of the four conditions alone skips the registration, none of them does not.
// Built by tests/test_lm_rows.py with -ffp-contract=off and AddressSanitizer + UBSan as a program of its own.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_rows.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() { uint64_t z = (g_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same3(const double a[3], const double b[3]) { return same(a[0], b[0]) && same(a[1], b[1]) && same(a[2], b[2]); }

struct In { bool edge; double a[3], b[3], d; float4 pt; };

// a row whose residual at `truth` is about `off` (an edge through two points at that distance from the mapped query; a plane at that distance)
static In make_row(bool edge, const double truth[6], double off, bool zero_d) {
  In r{};
  r.edge = edge;
  r.pt = float4{(float)uni(-40, 40), (float)uni(-40, 40), (float)uni(-3, 6), (float)uni(0, 16)};
  const double cp[3] = {r.pt.x, r.pt.y, r.pt.z};
  const PoseTerms T = pose_terms(truth);
  double lp[3];
  dq_rotate(T.q, cp, lp);
  for (int k = 0; k < 3; ++k) lp[k] += T.t[k];
  double n[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)}, u[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
  const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int k = 0; k < 3; ++k) n[k] /= nn;
  const double dot = u[0] * n[0] + u[1] * n[1] + u[2] * n[2];
  for (int k = 0; k < 3; ++k) u[k] -= dot * n[k];
  const double un = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; ++k) u[k] /= un;
  if (edge) {
    for (int k = 0; k < 3; ++k) { const double base = lp[k] + off * n[k]; r.a[k] = base + 0.1 * u[k]; r.b[k] = base - 0.1 * u[k]; }
    r.d = 0.0;
  } else {
    for (int k = 0; k < 3; ++k) r.a[k] = n[k];
    r.d = zero_d ? 0.0 : -(n[0] * lp[0] + n[1] * lp[1] + n[2] * lp[2]) + off;
  }
  return r;
}

// n doubles at a 16-byte boundary (what the block and streamed records have on the device)
struct Aligned {
  std::vector<double> v;
  double* p;
  explicit Aligned(size_t n, double fill = 0.0) : v(n + 2, fill), p(v.data() + ((reinterpret_cast<uintptr_t>(v.data()) & 15) ? 1 : 0)) {}
};

static void check_edge(const LmEdge& e, const In& r, const char* via) {
  const double p[3] = {r.pt.x, r.pt.y, r.pt.z};
  CHECK(same3(e.a, r.a) && same3(e.b, r.b) && same3(e.p, p), "edge read back %s differs from the input", via);
}
static void check_plane(const LmPlane& q, const In& r, const char* via) {
  const double p[3] = {r.pt.x, r.pt.y, r.pt.z};
  CHECK(same3(q.n, r.a) && same(q.d, r.d) && same3(q.p, p), "plane read back %s differs from the input", via);
}

static void test_layout(const std::vector<In>& rows) {
  // the query-to-row mapping: a corner query q has row q, a surf query q row surf_row0 + q
  CHECK(lm_row_of(0, 7, 100) == 7 && lm_row_of(1, 7, 100) == 107 && lm_row_of(1, 0, 100) == 100, "lm_row_of");
  CHECK(lm_row_of_query(4, 5, 100) == 4 && lm_row_of_query(5, 5, 100) == 100 && lm_row_of_query(9, 5, 100) == 104, "lm_row_of_query");
  int Rc = 0, Rs = 0;
  for (const In& r : rows) (r.edge ? Rc : Rs) += 1;
  // every row resident, and a second set of LDS arrays that holds the first edge and the first plane alone
  Aligned lds_all((60 * (size_t)Rc + 44 * (size_t)Rs + 7) / 8), lds_one(13);
  Aligned crows((size_t)(Rc + Rs) * 10, -7.0);
  const LmRows Wall = lml_make(Rc, Rs, reinterpret_cast<unsigned char*>(lds_all.p), 60 * (size_t)Rc + 44 * (size_t)Rs, crows.p);
  const LmRows Wone = lml_make(Rc, Rs, reinterpret_cast<unsigned char*>(lds_one.p), 104, crows.p);
  CHECK(Wall.Ce == Rc && Wall.Cp == Rs && Wone.Ce == 1 && Wone.Cp == 1 && Wone.Rc == Rc && Wone.Rs == Rs && Wone.crows == crows.p, "resident counts %d %d %d %d", Wall.Ce, Wall.Cp, Wone.Ce, Wone.Cp);
  int ie = 0, ip = 0;
  for (const In& r : rows) {
    alignas(16) double blk[8] = {-1, -2, -3, -4, -5, -6, -7, -8};
    if (r.edge) lmb_put_edge(blk, r.a, r.b); else lmb_put_plane(blk, r.a, r.d);
    // the block record, written out
    CHECK(same(blk[0], r.a[0]) && same(blk[1], r.a[1]) && same(blk[2], r.a[2]), "block [0..2]");
    if (r.edge) CHECK(same(blk[3], r.b[0]) && same(blk[4], r.b[1]) && same(blk[5], r.b[2]) && same(blk[6], 0.0) && same(blk[7], 2.0), "edge block [3..7]");
    else CHECK(same(blk[3], 0.0) && same(blk[4], 0.0) && same(blk[5], 0.0) && same(blk[6], r.d) && same(blk[7], 3.0), "plane block [3..7]");
    const LmBlock B = lmb_load(blk);
    CHECK(lmb_type(B) == (r.edge ? (double)BLK_EDGE : (double)BLK_PLANE), "lmb_type");
    // reader 1: block + point
    if (r.edge) check_edge(lm_edge_of(B, r.pt), r, "from the block"); else check_plane(lm_plane_of(B, r.pt), r, "from the block");
    // the streamed record: edges from record 0, planes from record Rc
    const size_t at = r.edge ? lms_edge_at(ie) : lms_plane_at(Rc, ip);
    CHECK(at == (size_t)(r.edge ? ie : Rc + ip), "record index");
    double* rec = crows.p + at * 10;
    lms_put(rec, B, r.pt);
    for (int k = 0; k < 8; ++k) CHECK(same(rec[k], blk[k]), "streamed record [%d]", k);
    float f[4];
    std::memcpy(f, rec + 8, sizeof f);
    CHECK(std::memcmp(f, &r.pt, sizeof f) == 0, "streamed record: float4 at double 8");
    if (r.edge) check_edge(lms_edge(rec), r, "from the streamed record"); else check_plane(lms_plane(rec), r, "from the streamed record");
    // the LDS arrays
    if (r.edge) { lml_put_edge(Wall, ie, B, r.pt); if (ie < Wone.Ce) lml_put_edge(Wone, ie, B, r.pt); ++ie; }
    else { lml_put_plane(Wall, ip, B, r.pt); if (ip < Wone.Cp) lml_put_plane(Wone, ip, B, r.pt); ++ip; }
  }
  // reader 3, after every row has been written (a writer that strays into a neighbour's field shows here)
  ie = ip = 0;
  for (const In& r : rows) {
    if (r.edge) { check_edge(lml_edge(Wall, ie), r, "from LDS"); if (ie < 1) check_edge(lml_edge(Wone, ie), r, "from LDS (one resident)"); ++ie; }
    else { check_plane(lml_plane(Wall, ip), r, "from LDS"); if (ip < 1) check_plane(lml_plane(Wone, ip), r, "from LDS (one resident)"); ++ip; }
  }
  // the arrays, written out: ea | eb (3 Ce each), pn (4 Cp), then ep (3 Ce) and pp (3 Cp) as f32
  const double* base = lds_all.p;
  const float* fbase = reinterpret_cast<const float*>(base + 6 * Rc + 4 * Rs);
  ie = ip = 0;
  for (const In& r : rows) {
    if (r.edge) {
      for (int k = 0; k < 3; ++k) CHECK(same(base[k * Rc + ie], r.a[k]) && same(base[3 * Rc + k * Rc + ie], r.b[k]), "LDS ea / eb");
      CHECK(fbase[ie] == r.pt.x && fbase[Rc + ie] == r.pt.y && fbase[2 * Rc + ie] == r.pt.z, "LDS ep");
      ++ie;
    } else {
      for (int k = 0; k < 3; ++k) CHECK(same(base[6 * Rc + k * Rs + ip], r.a[k]), "LDS pn");
      CHECK(same(base[6 * Rc + 3 * Rs + ip], r.d), "LDS pn (d)");
      CHECK(fbase[3 * Rc + ip] == r.pt.x && fbase[3 * Rc + Rs + ip] == r.pt.y && fbase[3 * Rc + 2 * Rs + ip] == r.pt.z, "LDS pp");
      ++ip;
    }
  }
  alignas(16) double blk[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  lmb_put_none(blk);
  CHECK(blk[7] == 0.0 && lmb_type(lmb_load(blk)) == 0.0, "a rejected query's type");
}

static void test_split() {
  const int counts[4] = {0, 1, 2, 5};
  for (int Rc : counts)
    for (int Rs : counts) {
      const long budgets[] = {0, 43, 44, 59, 60, 61, 103, 104, 60L * Rc - 1, 60L * Rc, 60L * Rc + 43, 60L * Rc + 44L * Rs, 60L * Rc + 44L * Rs + 1000};
      for (long b : budgets) {
        if (b < 0) continue;   // (60 Rc - 1 at Rc = 0)
        int Ce = -1, Cp = -1;
        lml_split(Rc, Rs, (size_t)b, &Ce, &Cp);
        const long we = b / 60 < Rc ? b / 60 : Rc, wp = (b - 60 * we) / 44 < Rs ? (b - 60 * we) / 44 : Rs;
        CHECK(Ce == we && Cp == wp, "split Rc %d Rs %d budget %ld: %d %d, want %ld %ld", Rc, Rs, b, Ce, Cp, we, wp);
        const LmLdsOff o = lml_offsets(Ce, Cp);
        CHECK(o.ea == 0 && o.eb == o.ea + 24u * Ce && o.pn == o.eb + 24u * Ce && o.ep == o.pn + 32u * Cp && o.pp == o.ep + 12u * Ce && o.end == o.pp + 12u * Cp, "arrays back to back");
        CHECK(o.end <= (size_t)b, "arrays end at %zu beyond the budget %ld", o.end, b);
        CHECK(o.ea % 8 == 0 && o.eb % 8 == 0 && o.pn % 8 == 0, "f64 arrays at multiples of 8 bytes");
      }
    }
}

static void test_evaluators(const std::vector<In>& rows, const double x[6], double huber) {
  const PoseTerms T = pose_terms(x);
  const double c3[3] = {0, 0, 0};
  double want[28] = {0}, got[28] = {0}, want_cost[28] = {0}, got_cost[28] = {0};
  int inl = 0, outl = 0;
  for (const In& r : rows) {
    const double cp[3] = {r.pt.x, r.pt.y, r.pt.z};
    double res, J[6];
    if (r.edge) {
      eval_block(BLK_EDGE, cp, r.a, r.b, c3, 0.0, T, &res, J);
      accumulate_block(res, J, huber, want);
      accumulate_cost(eval_block_residual<BLK_EDGE>(cp, r.a, r.b, c3, 0.0, T), huber, want_cost[27]);
      const LmEdge e{{r.a[0], r.a[1], r.a[2]}, {r.b[0], r.b[1], r.b[2]}, {cp[0], cp[1], cp[2]}};
      lm_eval_edge<true>(e, T, huber, got);
      lm_eval_edge<false>(e, T, huber, got_cost);
    } else {
      eval_block(BLK_PLANE, cp, r.a, c3, c3, r.d, T, &res, J);
      accumulate_block(res, J, huber, want);
      accumulate_cost(eval_block_residual<BLK_PLANE>(cp, r.a, c3, c3, r.d, T), huber, want_cost[27]);
      const LmPlane p{{r.a[0], r.a[1], r.a[2]}, r.d, {cp[0], cp[1], cp[2]}};
      lm_eval_plane<true>(p, T, huber, got);
      lm_eval_plane<false>(p, T, huber, got_cost);
    }
    (fabs(res) > huber ? outl : inl) += 1;
    for (int k = 0; k < 28; ++k) CHECK(same(want[k], got[k]), "normal equations, scalar %d after a row", k);
    for (int k = 0; k < 28; ++k) CHECK(same(want_cost[k], got_cost[k]), "cost-only, scalar %d after a row (only 27 may move)", k);
  }
  CHECK(same(want[27], want_cost[27]), "the cost of the full and of the cost-only evaluation");
  CHECK(inl > 10 && outl > 10, "rows on both sides of the Huber delta: %d inside, %d beyond", inl, outl);
}

static void test_guard() {
  // (ncur_c, ntotal, kds_c, no_map) against the minima 10, 100, 10
  CHECK(!lm_guard_fails(10, 100, 10, false, 10, 100, 10), "nothing fails: the registration runs");
  CHECK(lm_guard_fails(9, 100, 10, false, 10, 100, 10), "too few corner points");
  CHECK(lm_guard_fails(10, 99, 10, false, 10, 100, 10), "too few surf points");
  CHECK(lm_guard_fails(10, 100, 9, false, 10, 100, 10), "too small a corner map");
  CHECK(lm_guard_fails(10, 100, 10, true, 10, 100, 10), "no map yet");
  CHECK(lm_guard_fails(0, 0, 0, true, 10, 100, 10), "everything fails");
}

int main() {
  const double truth[6] = {0.4, -0.3, 0.05, 0.01, -0.02, 0.3}, x[6] = {0.41, -0.29, 0.06, 0.011, -0.018, 0.301};
  const double huber = 0.1;
  std::vector<In> rows;
  for (int i = 0; i < 200; ++i) {
    const bool edge = (next_u64() & 1) != 0;
    const double off = (i % 2) ? uni(-0.05, 0.05) : (uni(0, 1) < 0.5 ? -1.0 : 1.0) * uni(0.2, 1.5);   // inside / beyond the Huber delta
    rows.push_back(make_row(edge, truth, off, false));
  }
  rows.push_back(make_row(false, truth, 0.0, true));   // a plane through the origin: d = 0
  rows.push_back(make_row(true, truth, 0.0, false));
  test_layout(rows);
  test_split();
  test_evaluators(rows, x, huber);
  test_guard();
  if (g_fail) { std::printf("lm_rows FAILED: %d of %ld checks\n", g_fail, g_checks); return 1; }
  std::printf("lm_rows ok: %ld checks, %zu rows\n", g_checks, rows.size());
  return 0;
}
