// Stand-alone check of csrc/merge_math.h, the arithmetic of alego_map_move / alego_map_merge that kernels and host twins share
// (tests/test_map_merge.py builds it with -fsanitize=address,undefined and runs it): the moved pose, the moved prior, the seam, the shifted
// edges and the finiteness test, against values written out here.  The header must be readable by a host compiler without the HIP runtime.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "merge_math.h"

namespace {
int checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }
void yaw_T(double yaw, double x, double y, double z, double* T) {
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double M[12] = {c, -s, 0, x, s, c, 0, y, 0, 0, 1, z};
  std::memcpy(T, M, sizeof(M));
}
}  // namespace

int main() {
  const double kPi = 3.14159265358979323846;
  // (a) the moved pose: the identity returns the conversion alone; a yaw and a translation add up; G then G^-1 returns
  {
    double I[12], G[12], Gi[12];
    yaw_T(0.0, 0, 0, 0, I);
    const float kp[6] = {3.f, -2.f, 0.5f, 0.01f, -0.02f, 0.7f};
    float o[6], b[6];
    mg_move_pose6(I, kp, o);
    for (int k = 0; k < 6; ++k) CHECK(near(o[k], kp[k], 1e-6));
    yaw_T(0.5, 10, 20, 1, G);
    mg_move_pose6(G, kp, o);
    CHECK(near(o[0], 10 + std::cos(0.5) * 3 + std::sin(0.5) * 2, 1e-5) && near(o[1], 20 + std::sin(0.5) * 3 - std::cos(0.5) * 2, 1e-5) && near(o[2], 1.5, 1e-6));
    CHECK(near(o[5], 1.2, 1e-6) && near(o[3], kp[3], 1e-6) && near(o[4], kp[4], 1e-6));
    yaw_T(-0.5, -(std::cos(0.5) * 10 + std::sin(0.5) * 20), -(-std::sin(0.5) * 10 + std::cos(0.5) * 20), -1, Gi);
    mg_move_pose6(Gi, o, b);
    for (int k = 0; k < 6; ++k) CHECK(near(b[k], kp[k], 2e-6 * 25));
    mg_move_pose6(I, kp, o);
    float same[6];
    std::memcpy(same, kp, sizeof(same));
    mg_move_pose6(I, same, same);   // in place
    CHECK(std::memcmp(same, o, sizeof(o)) == 0);
    // a yaw across the branch cut stays in (-pi, pi]
    const float back[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 3.0f};
    mg_move_pose6(G, back, o);
    CHECK(near(o[5], 3.5 - 2 * kPi, 1e-6));
  }
  // (b) the moved prior is T * between, in place too
  {
    double G[12], B[12], O[12];
    yaw_T(kPi / 2, 1, 2, 3, G);
    yaw_T(0.0, 5, 0, 0, B);
    mg_move_prior(G, B, O);
    CHECK(near(O[3], 1, 1e-12) && near(O[7], 7, 1e-12) && near(O[11], 3, 1e-12) && near(O[1], -1, 1e-12) && near(O[4], 1, 1e-12));
    mg_move_prior(G, B, B);
    CHECK(std::memcmp(B, O, sizeof(O)) == 0);
  }
  // (c) the seam: the prior for an empty destination, else between(previous, first); the variances are the seam's
  {
    const float prev[6] = {1.f, 0.f, 0.f, 0.f, 0.f, (float)(kPi / 2)}, first[6] = {1.f, 2.f, 0.f, 0.f, 0.f, (float)(kPi / 2)};
    const double var[6] = {1, 2, 3, 4, 5, 6};
    alego_graph_edge e;
    mg_seam_edge(0, nullptr, first, var, &e);
    CHECK(e.from == -1 && e.to == 0 && near(e.between[3], 1, 1e-7) && near(e.between[7], 2, 1e-7) && near(e.between[4], 1, 1e-7));
    mg_seam_edge(7, prev, first, var, &e);
    CHECK(e.from == 6 && e.to == 7);
    CHECK(near(e.between[3], 2, 1e-6) && near(e.between[7], 0, 1e-6) && near(e.between[0], 1, 1e-7) && near(e.between[5], 1, 1e-7));   // two metres ahead, same heading
    for (int k = 0; k < 6; ++k) CHECK(e.variance[k] == var[k]);
  }
  // (d) shifted edges keep every byte but the ids
  {
    std::vector<alego_graph_edge> in(3), out(3);
    for (int i = 0; i < 3; ++i) {
      in[i].from = i - 1; in[i].to = i;
      for (int k = 0; k < 12; ++k) in[i].between[k] = 0.1 * i + k;
      for (int k = 0; k < 6; ++k) in[i].variance[k] = 1e-6 * (k + 1);
    }
    for (int i = 0; i < 3; ++i) mg_shift_edge(&in[i], 40, &out[i]);
    for (int i = 0; i < 3; ++i) {
      CHECK(out[i].from == in[i].from + 40 && out[i].to == in[i].to + 40);
      CHECK(std::memcmp(out[i].between, in[i].between, sizeof(in[i].between)) == 0 && std::memcmp(out[i].variance, in[i].variance, sizeof(in[i].variance)) == 0);
    }
    mg_shift_edge(&in[2], 0, &in[2]);   // in place, no shift
    CHECK(in[2].from == 1 && in[2].to == 2);
  }
  // (e) finiteness
  {
    double G[12];
    yaw_T(0.1, 1, 2, 3, G);
    CHECK(mg_finite12(G));
    G[5] = std::numeric_limits<double>::quiet_NaN();
    CHECK(!mg_finite12(G));
    G[5] = 1.0; G[11] = -std::numeric_limits<double>::infinity();
    CHECK(!mg_finite12(G));
  }
  CHECK(MG_ITEM == ALEGO_MERGE_COPY_ITEM && MG_ITEM == 4 * MG_T);
  std::printf("merge_math ok: %d checks\n", checks);
  return 0;
}
