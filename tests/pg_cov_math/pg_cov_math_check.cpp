// Stand-alone run of csrc/pg_cov_math.h, the arithmetic of the key-pose graph's marginal covariances and of the loop-edge gate that the device
// kernels and the host twin share (tests/test_graph_cov.py builds it with -fsanitize=address,undefined, writes the cases and compares the
// output with numpy's dense inverse).  The header must be readable by a host compiler without the HIP runtime.
//
//   pg_cov_math_check CASES   CASES: per case, every real number as a C99 hexadecimal float (exact in both directions):
//                               n_poses n_edges n_pairs n_cand / poses[n_poses][12] / per edge: from to between[12] variance[6] (chain first) /
//                               per pair: i j / per candidate: from to between[12] variance[6]
//   prints per case           marginals[n_poses][36]  pairs[n_pairs][36]  per candidate: status d2 error[6] P[36];  "pg_cov_math ok <cases>" at the end
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pg_cov_math.h"

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
