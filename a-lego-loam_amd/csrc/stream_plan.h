// stream_plan.h — how many HIP streams a handle drives, fitted to the hardware queues of the process.  Plain C++ (no HIP include): the
// host API (alego_api.hip) and a CPU test program (tests/stream_plan) compile the same definition.
//
// A handle splits its slots into G contiguous stream groups, one HIP stream each, and may give every group a second ("back") stream on which
// LaserMapping of scan k runs while the group's front end works on scans k + 1, k + 2: G x (1 + async) streams.  The HIP runtime maps streams
// onto the process's hardware queues, and streams that share a queue serialise — an overlap the plan asks for and the queues cannot give costs
// more than it is worth.  So whatever the caller did not ask for explicitly is chosen to fit: G x (1 + async) <= Q.
//
//   Q       ALEGO_HW_QUEUES, else GPU_MAX_HW_QUEUES (read, never set), else 4 (the HIP runtime's default)
//   groups  ALEGO_STREAM_GROUPS when set (1 .. 8), else n_slots / 64 capped at 4 (and at kGroupCap[Q] below 8 queues)
//   async   ALEGO_LM_ASYNC when set, else 1 where the groups leave room for their back streams (2 G <= Q)
//
// With Q >= 8 and no request the plan is what the library always did (up to 4 groups, a back stream each).  Both requests given are taken as
// they are at any Q: ALEGO_STREAM_GROUPS=4 ALEGO_LM_ASYNC=1 is the plan of the rounds before the fit, whatever the queues.
#pragma once

#include <cstdlib>

struct StreamPlan {
  int groups;   // G: stream groups (front streams)
  int gsize;    // slots per group (the last group may hold fewer)
  int async;    // 1: every group has a back stream for LaserMapping
  int queues;   // Q the plan was fitted to
};

constexpr int STREAM_PLAN_MAX_GROUPS = 8;       // an explicit request is cut here
constexpr int STREAM_PLAN_DEFAULT_GROUPS = 4;   // the default asks for no more
constexpr int STREAM_PLAN_FULL_QUEUES = 8;      // from here on the default plan fits as it is
constexpr int STREAM_PLAN_DEFAULT_QUEUES = 4;   // HIP's own default when the environment names none

// Below 8 queues groups and back streams compete for them: kGroupCap[Q] is the number of groups the default plan may take at Q; the back
// streams follow where 2 G <= Q still holds.  Every entry measured at 4 096 streams of 16 x 1800 (profiles/r07_stream_plan.md): plain groups
// beat fewer groups with back streams at every Q below 8, and more groups than queues lose again (Q = 2: 2 groups 461 k scans/s, 4 groups 443 k).
constexpr int kGroupCap[STREAM_PLAN_FULL_QUEUES] = {1, 1, 2, 3, 4, 4, 4, 4};

// Q from the two environment values (nullptr = not set); values below 1 or not a number count as not set
inline int stream_plan_queues(const char* alego_hw_queues, const char* gpu_max_hw_queues) {
  const char* const src[2] = {alego_hw_queues, gpu_max_hw_queues};
  for (const char* e : src) {
    if (!e) continue;
    const int q = std::atoi(e);
    if (q >= 1) return q;
  }
  return STREAM_PLAN_DEFAULT_QUEUES;
}

// groups -> (groups, gsize) covering n_slots with contiguous groups of equal size, none empty
inline void stream_plan_cover(int n_slots, int G, StreamPlan* p) {
  if (G > n_slots) G = n_slots;
  if (G < 1) G = 1;
  p->gsize = (n_slots + G - 1) / G;
  p->groups = (n_slots + p->gsize - 1) / p->gsize;
}

// req_groups / req_async: the explicit requests, < 0 = none
inline StreamPlan stream_plan(int n_slots, int Q, int req_groups, int req_async) {
  StreamPlan p;
  if (n_slots < 1) n_slots = 1;
  if (Q < 1) Q = 1;
  p.queues = Q;
  int G;
  if (req_groups >= 0) {
    G = req_groups > STREAM_PLAN_MAX_GROUPS ? STREAM_PLAN_MAX_GROUPS : req_groups;
  } else {
    G = n_slots / 64;
    if (G > STREAM_PLAN_DEFAULT_GROUPS) G = STREAM_PLAN_DEFAULT_GROUPS;
    if (G < 1) G = 1;
    int cap = Q < STREAM_PLAN_FULL_QUEUES ? kGroupCap[Q] : STREAM_PLAN_DEFAULT_GROUPS;
    if (req_async > 0 && cap > Q / 2) cap = Q / 2 > 1 ? Q / 2 : 1;   // the back streams were asked for: the groups make room
    if (G > cap) G = cap;
  }
  stream_plan_cover(n_slots, G, &p);
  p.async = req_async >= 0 ? (req_async != 0) : (2 * p.groups <= Q);
  return p;
}

// alego_stream_run drives three chains (ImageProjection + feature extraction ahead, LaserOdometry, LaserMapping) on min(3, Q) streams;
// the handle's front stream and, where it has one, its back stream are among them.  Returns how many streams the run uses in all.
inline int stream_plan_lookahead_streams(int Q, int have) {
  int want = Q < 3 ? (Q < 1 ? 1 : Q) : 3;
  return want > have ? want : have;
}
