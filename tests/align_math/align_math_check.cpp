// Stand-alone check of csrc/align_math.h, the rule of alego_map_align that kernel and host share (tests/test_map_align.py builds it with
// -fsanitize=address,undefined and runs it): the query frames, the agreement of two hypotheses, the order of fitness keys and the consensus,
// against values written out here.  The header must be readable by a host compiler without the HIP runtime.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "align_math.h"

namespace {
int checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
struct Hyp { float T[16]; float p[3]; };
Hyp yaw_at(double yaw, double x, double y, double z, float px = 0.f, float py = 0.f, float pz = 0.f) {
  Hyp h{};
  const float c = (float)std::cos(yaw), s = (float)std::sin(yaw);
  const float T[16] = {c, -s, 0, (float)x, s, c, 0, (float)y, 0, 0, 1, (float)z, 0, 0, 0, 1};
  for (int i = 0; i < 16; ++i) h.T[i] = T[i];
  h.p[0] = px; h.p[1] = py; h.p[2] = pz;
  return h;
}
}  // namespace

int main() {
  // (a) the queries: distinct, ascending, inside [0, ns), the middle of equal stretches
  for (int nq : {1, 8, 32})
    for (int ns : {0, 1, 2, nq - 1, nq, nq + 1, 1000, 1 << 24}) {
      if (ns < 0) continue;
      const int Q = ma_query_count(ns, nq);
      CHECK(Q == (ns < nq ? ns : nq));
      int last = -1;
      for (int q = 0; q < Q; ++q) {
        const int f = ma_query_frame(ns, Q, q);
        CHECK(f > last && f >= 0 && f < ns);
        CHECK((long long)f * Q <= (long long)q * ns + ns / 2 && (long long)(f + 1) * Q > (long long)q * ns);   // inside stretch q
        last = f;
      }
    }
  CHECK(ma_query_frame(1000, 8, 0) == 62 && ma_query_frame(1000, 8, 7) == 937 && ma_query_frame(5, 5, 4) == 4 && ma_query_frame(1, 1, 0) == 0);
  // (b) agreement: itself, a small and a large difference, symmetric, positions rather than translation columns, non-finite
  const Hyp a = yaw_at(0.3, 10, -4, 1, 5, 6, 0), b = yaw_at(0.31, 10.05, -4, 1, -3, 2, 0), far = yaw_at(0.3 + 3.14159, 30, 9, 1);
  CHECK(ma_agree(a.T, a.p, a.T, a.p, 0.0, 0.0) || ma_agree(a.T, a.p, a.T, a.p, 1e-12, 1e-7));   // (f32 entries: R^T R is the identity to rounding)
  CHECK(ma_agree(a.T, a.p, b.T, b.p, 0.5, 0.05) && ma_agree(b.T, b.p, a.T, a.p, 0.5, 0.05));
  CHECK(!ma_agree(a.T, a.p, b.T, b.p, 0.5, 0.005) && !ma_agree(a.T, a.p, b.T, b.p, 0.01, 0.05));
  CHECK(!ma_agree(a.T, a.p, far.T, far.p, 0.5, 0.05) && !ma_agree(far.T, far.p, a.T, a.p, 0.5, 0.05));
  const Hyp o1 = yaw_at(0.0, 1, 2, 3, 100, 0, 0), o2 = yaw_at(0.003, 1, 2, 3, 0, 100, 0), o3 = yaw_at(0.003, 1, 2, 3, 0, 0, 0), o4 = yaw_at(0.0, 1, 2, 3);
  CHECK(!ma_agree(o1.T, o1.p, o2.T, o2.p, 0.25, 0.02));   // 0.003 rad at 100 m: 0.3 m
  CHECK(ma_agree(o4.T, o4.p, o3.T, o3.p, 0.25, 0.02));    // the same two transforms seen from the origin
  Hyp bad = a;
  bad.T[3] = std::numeric_limits<float>::quiet_NaN();
  CHECK(!ma_agree(bad.T, bad.p, bad.T, bad.p, 1e9, 4.0) && !ma_agree(a.T, a.p, bad.T, bad.p, 1e9, 4.0));
  bad = a;
  bad.T[0] = std::numeric_limits<float>::infinity();
  CHECK(!ma_agree(bad.T, bad.p, bad.T, bad.p, 1e9, 4.0) && !ma_agree(bad.T, bad.p, a.T, a.p, 1e9, 4.0));
  // (c) the fitness key orders as `<` does
  const double fs[] = {-1.0, -0.0, 0.0, 1e-300, 0.1, 0.1000000000000001, 1.0, 1e300, std::numeric_limits<double>::infinity()};
  for (double x : fs)
    for (double y : fs)
      if (!(x == 0.0 && y == 0.0)) CHECK((ma_fit_key(x) < ma_fit_key(y)) == (x < y));
  // (d) the consensus: two disjoint agreeing pairs, the fitness breaks the tie and then the index; not accepted, not finite
  std::vector<Hyp> H = {yaw_at(0, 0, 0, 0), yaw_at(0, 50, 0, 0), yaw_at(0.001, 0.01, 0, 0), yaw_at(0.001, 50.01, 0, 0), yaw_at(1.0, -70, 0, 0)};
  std::vector<float> T, P;
  for (const Hyp& h : H) { T.insert(T.end(), h.T, h.T + 16); P.insert(P.end(), h.p, h.p + 3); }
  int32_t sup[8];
  {
    const double fit[5] = {0.2, 0.1, 0.3, 0.4, 0.01};
    const int32_t acc[5] = {1, 1, 1, 1, 1};
    CHECK(ma_consensus_ref(T.data(), P.data(), fit, acc, 5, 0.25, 0.02, sup) == 1);
    CHECK(sup[0] == 2 && sup[1] == 2 && sup[2] == 2 && sup[3] == 2 && sup[4] == 1);
    const double same[5] = {0.1, 0.1, 0.1, 0.1, 0.1};
    CHECK(ma_consensus_ref(T.data(), P.data(), same, acc, 5, 0.25, 0.02, sup) == 0);
    const int32_t one[5] = {0, 0, 0, 0, 1};
    CHECK(ma_consensus_ref(T.data(), P.data(), fit, one, 5, 0.25, 0.02, sup) == 4 && sup[4] == 1 && sup[0] == 0);
    const int32_t none[5] = {0, 0, 0, 0, 0};
    CHECK(ma_consensus_ref(T.data(), P.data(), fit, none, 5, 0.25, 0.02, sup) == -1 && sup[2] == 0);
    CHECK(ma_consensus_ref(T.data(), P.data(), fit, acc, 0, 0.25, 0.02, sup) == -1);
    T[3] = std::numeric_limits<float>::quiet_NaN();
    CHECK(ma_consensus_ref(T.data(), P.data(), same, acc, 5, 0.25, 0.02, sup) == 1 && sup[0] == 0 && sup[2] == 1);
  }
  std::printf("align_math ok: %d checks\n", checks);
  return 0;
}
