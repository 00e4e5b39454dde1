// Prints what csrc/stream_plan.h decides, one line per case, for tests/test_stream_plan.py (which holds the expectations).
//   plan  <Q> <n_slots> <req_groups> <req_async> -> <groups> <gsize> <async> <queues>
//   queue <ALEGO_HW_QUEUES or -> <GPU_MAX_HW_QUEUES or -> -> <Q>
//   look  <Q> <streams the handle has> -> <streams alego_stream_run uses>
#include <cstdio>

#include "stream_plan.h"

int main() {
  const int slots[] = {1, 3, 5, 63, 64, 255, 256, 4096};
  for (int Q = 1; Q <= 32; ++Q)
    for (int n : slots)
      for (int rg = -1; rg <= 9; ++rg)
        for (int ra = -1; ra <= 1; ++ra) {
          const StreamPlan p = stream_plan(n, Q, rg, ra);
          std::printf("plan %d %d %d %d -> %d %d %d %d\n", Q, n, rg, ra, p.groups, p.gsize, p.async, p.queues);
        }
  const char* vals[] = {nullptr, "0", "1", "2", "4", "8", "32", "x", "-3"};
  for (const char* a : vals)
    for (const char* g : vals)
      std::printf("queue %s %s -> %d\n", a ? a : "-", g ? g : "-", stream_plan_queues(a, g));
  for (int Q = 1; Q <= 8; ++Q)
    for (int have = 1; have <= 2; ++have) std::printf("look %d %d -> %d\n", Q, have, stream_plan_lookahead_streams(Q, have));
  std::printf("stream_plan ok\n");
  return 0;
}
