// Stand-alone check of csrc/thin_math.h, the rule of alego_map_thin that the kernels and the host twins share (tests/test_map_thin.py builds it
// with -fsanitize=address,undefined and runs it): the threshold, the greedy selection at its edges, the composed chain edge and the remapped
// loop edge, against values written out here.  The header must be readable by a host compiler without the HIP runtime.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "thin_math.h"

namespace {
int checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
std::vector<uint8_t> select(const std::vector<float>& xyz, const std::vector<uint8_t>& protect, double min_dist, int* kept = nullptr) {
  const int n = (int)xyz.size() / 3;
  std::vector<float> kp((size_t)n * 6, 0.f);
  for (int i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) kp[(size_t)i * 6 + k] = xyz[(size_t)i * 3 + k];
  std::vector<uint8_t> keep((size_t)n, 7);
  const int c = th_select_host(kp.data(), 6, protect.empty() ? nullptr : protect.data(), n, min_dist, keep.data());
  if (kept) *kept = c;
  return keep;
}
alego_graph_edge edge(int from, int to, double yaw, double x, double y, double z, double v0) {
  alego_graph_edge e;
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double M[12] = {c, -s, 0, x, s, c, 0, y, 0, 0, 1, z};
  std::memcpy(e.between, M, sizeof(M));
  for (int k = 0; k < 6; ++k) e.variance[k] = v0 * (k + 1);
  e.from = from; e.to = to;
  return e;
}
}  // namespace

int main() {
  typedef std::vector<uint8_t> M;
  // (a) the threshold: (float)(d * d), and a value no squared distance is below when nothing is dropped
  CHECK(th_r2(3.0) == 9.f && th_r2(0.0) == -1.f && th_r2(-2.0) == -1.f);
  CHECK(th_r2(0.1) == (float)(0.1 * 0.1));
  // (b) a pair at exactly r^2 stays, one step below it goes
  {
    int kept = 0;
    CHECK(select({0, 0, 0, 3, 4, 0}, {}, 5.0, &kept) == (M{1, 1}) && kept == 2);
    CHECK(select({0, 0, 0, 3, 4, 0}, {}, std::nextafter(5.0, 6.0)) == (M{1, 1}));   // (float)(r * r) is still 25
    CHECK(select({0, 0, 0, 3, 4, 0}, {}, 5.000001) == (M{1, 0}));
    CHECK(select({0, 0, 0, 3, 4, 0}, {0, 1}, 5.000001) == (M{1, 1}));
  }
  // (c) greedy: B is dropped by A and suppresses nobody, so C (close to B, far from A) stays
  CHECK(select({0, 0, 0, 2, 0, 0, 4, 0, 0}, {}, 3.0) == (M{1, 0, 1}));
  // (d) one place: frame 0 and the protected frames stay
  CHECK(select({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, {0, 0, 1, 0, 1}, 0.5) == (M{1, 0, 1, 0, 1}));
  // (e) a protected frame in the middle suppresses later frames
  CHECK(select({0, 0, 0, 10, 0, 0, 10, 1, 0, 0, 1, 0}, {0, 1, 0, 0}, 2.0) == (M{1, 1, 0, 0}));
  // (f) a NaN position: kept, suppresses nothing
  {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(select({0, 0, 0, nan, 0, 0, nan, 0, 0, 0, 0, 1}, {}, 2.0) == (M{1, 1, 1, 0}));
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(select({0, 0, 0, inf, 0, 0, inf, 0, 0}, {}, 2.0) == (M{1, 1, 1}));   // inf - inf is NaN
  }
  // (g) min_dist 0 and negative drop nothing; n = 1; n = 0
  CHECK(select({0, 0, 0, 0, 0, 0}, {}, 0.0) == (M{1, 1}) && select({0, 0, 0, 0, 0, 0}, {}, -5.0) == (M{1, 1}));
  CHECK(select({7, 8, 9}, {}, 100.0) == (M{1}) && select({}, {}, 1.0).empty());
  // (h) the composed edge: a run of one is the edge itself; a run of three is ((E1 E2) E3) with summed variances
  {
    std::vector<alego_graph_edge> ch = {edge(-1, 0, 0.3, 1, 2, 3, 1e-6), edge(0, 1, 0.1, 1, 0, 0, 1e-4), edge(1, 2, 0.2, 2, 0.5, 0, 2e-4), edge(2, 3, -0.4, 1, 1, 0.25, 4e-4)};
    alego_graph_edge o;
    th_compose_edge(ch.data(), 0, 1, 1, &o);
    CHECK(o.from == 0 && o.to == 1 && std::memcmp(o.between, ch[1].between, sizeof(o.between)) == 0 && std::memcmp(o.variance, ch[1].variance, sizeof(o.variance)) == 0);
    th_compose_edge(ch.data(), 0, 3, 1, &o);
    double a[12], b[12];
    pg_compose(ch[1].between, ch[2].between, a);
    pg_compose(a, ch[3].between, b);
    CHECK(o.from == 0 && o.to == 1 && std::memcmp(o.between, b, sizeof(b)) == 0);
    for (int k = 0; k < 6; ++k) CHECK(o.variance[k] == (ch[1].variance[k] + ch[2].variance[k]) + ch[3].variance[k]);
    // three planar edges: the yaws add up, the translation is t1 + R1 t2 + R1 R2 t3
    CHECK(std::fabs(std::atan2(o.between[4], o.between[0]) - (0.1 + 0.2 - 0.4)) < 1e-12);
    const double x = 1 + (std::cos(0.1) * 2 - std::sin(0.1) * 0.5) + (std::cos(0.3) * 1 - std::sin(0.3) * 1);
    CHECK(std::fabs(o.between[3] - x) < 1e-12 && std::fabs(o.between[11] - 0.25) < 1e-15);
    th_compose_edge(ch.data(), 1, 3, 2, &o);
    pg_compose(ch[2].between, ch[3].between, a);
    CHECK(o.from == 1 && o.to == 2 && std::memcmp(o.between, a, sizeof(a)) == 0);
  }
  // (i) the remapped loop edge
  {
    const int new_id[5] = {0, -1, 1, -1, 2};
    alego_graph_edge e = edge(4, 2, 0.5, 1, 1, 1, 1e-3), o;
    CHECK(th_remap_edge(&e, new_id, 5, &o) && o.from == 2 && o.to == 1 && std::memcmp(o.between, e.between, sizeof(e.between)) == 0 && std::memcmp(o.variance, e.variance, sizeof(e.variance)) == 0);
    e.from = 1;
    CHECK(!th_remap_edge(&e, new_id, 5, &o));
    e.from = 5;
    CHECK(!th_remap_edge(&e, new_id, 5, &o));
    e.from = -1;
    CHECK(!th_remap_edge(&e, new_id, 5, &o));
  }
  std::printf("thin_math ok (%d checks)\n", checks);
  return 0;
}
