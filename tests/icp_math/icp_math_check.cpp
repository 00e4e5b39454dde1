// Stand-alone run of csrc/icp_math.h, the per-iteration arithmetic that every ICP of the library shares (tests/test_icp_scenes.py builds it with
// -fsanitize=address,undefined, writes the cases and compares the output with an SVD reference in numpy).  The header must be readable by a
// host compiler without the HIP runtime.
//
//   icp_math_check CASES      CASES: one case per line, every number as a C99 hexadecimal float (exact in both directions):
//                             T[17]  prev_mse  iter  Tf[16]  icp_max_corr_dist  icp_max_iters  icp_trans_eps  icp_fitness_eps
//   prints per case           M[16]  Tf[16]  done  converged  iter  prev_mse  apply     after ONE icp_update, and "icp_math ok <cases>" at the end
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icp_math.h"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::vector<char> line(1 << 14);
  int cases = 0;
  while (std::fgets(line.data(), (int)line.size(), f)) {
    std::vector<double> v;
    char* s = line.data();
    while (true) {
      char* e = nullptr;
      const double x = std::strtod(s, &e);
      if (e == s) break;
      v.push_back(x);
      s = e;
    }
    if (v.empty()) continue;
    if (v.size() != 17 + 2 + 16 + 4) { std::fprintf(stderr, "case %d: %zu numbers\n", cases, v.size()); std::fclose(f); return 2; }
    double T[17];
    for (int k = 0; k < 17; ++k) T[k] = v[k];
    IcpState S;
    std::memset(&S, 0, sizeof(S));
    for (int k = 0; k < 16; ++k) { S.M[k] = (k % 5 == 0) ? 1.f : 0.f; S.Tf[k] = (float)v[19 + k]; }
    S.prev_mse = v[17]; S.fitness = DBL_MAX; S.iter = (int)v[18];
    alego_params P;
    alego_default_params(&P, 16, 1800);
    P.icp_max_corr_dist = v[35]; P.icp_max_iters = (int)v[36]; P.icp_trans_eps = v[37]; P.icp_fitness_eps = v[38];
    icp_update(&S, T, P);
    std::string out;
    char buf[64];
    for (int k = 0; k < 16; ++k) { std::snprintf(buf, sizeof(buf), "%a ", (double)S.M[k]); out += buf; }
    for (int k = 0; k < 16; ++k) { std::snprintf(buf, sizeof(buf), "%a ", (double)S.Tf[k]); out += buf; }
    std::snprintf(buf, sizeof(buf), "%d %d %d %a %d", S.done, S.converged, S.iter, S.prev_mse, S.apply);
    out += buf;
    std::puts(out.c_str());
    ++cases;
  }
  std::fclose(f);
  std::printf("icp_math ok %d\n", cases);
  return 0;
}
