// kernels_merge.hip — a slot moved by a rigid transform and one slot's key-frame archive appended to another's, on gfx950 (alego_map_move /
// alego_map_merge).  Both calls are defined by sequences of per-frame host calls (include/alego_mi355x.h) and leave the
// state those leave; the host (lm_host.hip) has checked every count before anything here is launched.
//
//   mg_copy         the hot path: the source's archived points, one contiguous range, behind the destination's.  A work list of (pair, item of
//                   MG_ITEM points): one big pair spreads over the device, a thousand small pairs take one launch.  One float4 (16 B) per lane and
//                   access, four accesses in flight per lane.
//   mg_frames       one lane per appended frame: its arc_tab row with the shifted point offset, the moved pose (merge_math.h), the stamp, and - with
//                   the graph on - its chain edge: the seam for the first frame, the source's edge with shifted ids for the others.  Lane 0 of a
//                   pair moves the destination's counters and clears its window as alego_lm_reset_window does.
//   mg_ring         the newest min(ns, K + 1) frames of the union go into the destination's ring rows (raw clouds, counts, pose) from the source's
//                   archive, as alego_lm_add_keyframe leaves them; mg_retransform + the key-frame sort jobs then run once per such frame, oldest
//                   first (lm_host.hip), as lm_host_graph_apply's rounds do.
//   mg_move         one workgroup per moved slot: archived and resident poses, the window, map -> odom, the prior of the chain.
// The source's loop edges and the hypotheses' cross edges go through graph_append / pg_append (kernels_graph.hip).
#include <hip/hip_runtime.h>

#include "../../include/alego_mi355x.h"
#include "dev_cost.h"
#include "kf_store.h"
#include "merge.h"
#include "merge_math.h"
#include "prof.h"

static_assert(MG_ITEM == 4 * MG_T, "mg_copy: four float4 per lane and item");

// grid (items), MG_T threads.  The host guarantees pd + ps <= arc_points_cap for every pair of the list.
__global__ void __launch_bounds__(MG_T) mg_copy(LmCtx L, const MgPair* pairs, const int2* items) {
  const int2 it = items[blockIdx.x];
  const MgPair& P = pairs[it.x];
  const float4* src = L.arc_pts + (size_t)P.src * L.arc_points_cap;
  float4* dst = L.arc_pts + (size_t)P.dst * L.arc_points_cap + P.pd;
  const int base = it.y * MG_ITEM + threadIdx.x, n = P.ps;
  // (four unconditional loads at clamped indices: a load under a condition sends the four values through LDS; n >= 1 for every item)
  const float4 v0 = src[min(base, n - 1)], v1 = src[min(base + MG_T, n - 1)], v2 = src[min(base + 2 * MG_T, n - 1)], v3 = src[min(base + 3 * MG_T, n - 1)];
  if (base < n) dst[base] = v0;
  if (base + MG_T < n) dst[base + MG_T] = v1;
  if (base + 2 * MG_T < n) dst[base + 2 * MG_T] = v2;
  if (base + 3 * MG_T < n) dst[base + 3 * MG_T] = v3;
}

// grid (ceil(ns_max / 64), pairs), 64 threads: lane f of pair blockIdx.y appends source frame f as frame nd + f of the destination
__global__ void __launch_bounds__(64) mg_frames(LmCtx L, const MgPair* pairs) {
  const MgPair& P = pairs[blockIdx.y];
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= P.ns) return;
  const int g = P.nd + f;
  const int* ts = arc_tab_of(L, P.src, f);
  int* td = arc_tab_of(L, P.dst, g);
  td[AT_OFF] = ts[AT_OFF] + P.pd;
#pragma unroll
  for (int k = 0; k < KF_KINDS; ++k) td[AT_N + k] = ts[AT_N + k];
  float kp[KF_POSE_W] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  mg_move_pose6(P.T, arc_pose_of(L, P.src, f), kp);
  float* pd = arc_pose_of(L, P.dst, g);
  for (int k = 0; k < KF_POSE_W; ++k) pd[k] = kp[k];
  L.arc_stamp[arc_row(L, P.dst, g)] = L.arc_stamp[arc_row(L, P.src, f)] + P.stamp_off;
  if (L.pg_loops_cap > 0) {
    alego_graph_edge* e = L.pg_chain + arc_row(L, P.dst, g);
    if (f == 0) mg_seam_edge(P.nd, P.nd > 0 ? arc_pose_of(L, P.dst, P.nd - 1) : kp, kp, P.seam_var, e);
    else mg_shift_edge(L.pg_chain + arc_row(L, P.src, f), P.nd, e);
  }
  if (f == 0) {
    int* st = arc_stat_of(L, P.dst);
    st[AS_FRAMES] = P.nd + P.ns; st[AS_POINTS] = P.pd + P.ps;
    int* li = L.li + (size_t)P.dst * LI_COUNT;
    li[LI_NKF] += P.ns;
    kf_reset_window([&](int w, int v) { li[w] = v; });
  }
}

// grid (tail_max, pairs), MG_T threads: the j-th oldest of the pair's `tail` newest frames into its ring row of the destination
__global__ void __launch_bounds__(MG_T) mg_ring(LmCtx L, const MgPair* pairs) {
  const MgPair& P = pairs[blockIdx.y];
  const int j = blockIdx.x;
  if (j >= P.tail) return;
  const int f = P.ns - P.tail + j, g = P.nd + f;
  const KfClouds C = kf_clouds(kf_arc_frame(L, P.src, f));
  const size_t row = kf_row(L, P.dst, g);
#pragma unroll
  for (int k = 0; k < KF_KINDS; ++k) {
    float4* raw = kf_raw_of(L, row, k);
    const int n = min(C.n[k], kf_cap_of(L, k));
    for (int i = threadIdx.x; i < n; i += MG_T) raw[i] = C.pts[k][i];
  }
  if (threadIdx.x < KF_POSE_W) kf_pose_of(L, row)[threadIdx.x] = arc_pose_of(L, P.dst, g)[threadIdx.x];   // (written by mg_frames, the launch before)
  if (threadIdx.x == 0) {
    int* cnt = kf_cnt_of(L, row);
    cnt[KF_CORNER] = C.n[KF_CORNER]; cnt[KF_SURF] = C.n[KF_SURF]; cnt[KF_OUTL] = C.n[KF_OUTL]; cnt[KF_KINDS] = 0;
  }
}

// grid (8, 3, slots of the group): kf_store.h's re-transform of one resident frame into kf_tmp_* for the key-frame sort jobs
__global__ void __launch_bounds__(MG_T) mg_retransform(LmCtx L, const int* tail, int slot0, int j) {
  const int slot = blockIdx.z + slot0, kind = blockIdx.y;
  const int t = tail[slot];
  if (j >= t) return;
  const int nkf = (L.li + (size_t)slot * LI_COUNT)[LI_NKF];
  if (nkf - t + j < 0) return;
  kf_row_to_tmp<MG_T>(L, slot, kf_entry(L, nkf - t + j), kind, false);
}

// grid (moved slots), MG_T threads
__global__ void __launch_bounds__(MG_T) mg_move(LmCtx L, const MgMove* moves) {
  const MgMove& M = moves[blockIdx.x];
  const int slot = M.slot;
  int* li = L.li + (size_t)slot * LI_COUNT;
  const int nkf = li[LI_NKF];
  for (int k = threadIdx.x; k < M.n; k += MG_T) {
    float kp[6];
    float* ap = arc_pose_of(L, slot, k);
    mg_move_pose6(M.T, ap, kp);
    for (int i = 0; i < 6; ++i) ap[i] = kp[i];
    if (k < nkf && k >= nkf - L.K) {
      float* rp = kf_pose_of(L, kf_row(L, slot, k));
      for (int i = 0; i < 6; ++i) rp[i] = kp[i];
    }
  }
  if (threadIdx.x == 0) {
    kf_reset_window([&](int w, int v) { li[w] = v; });
    double* ld = L.ld + (size_t)slot * LD_COUNT;
    dq_apply_correction(ld + LD_Q_M2O, ld + LD_T_M2O, M.T);
    if (L.pg_loops_cap > 0) {
      alego_graph_edge* e = L.pg_chain + arc_row(L, slot, 0);
      mg_move_prior(M.T, e->between, e->between);
    }
  }
}

void launch_mg_copy(const LmCtx& L, const MgPair* pairs, const int2* items, int n_items, hipStream_t st) {
  if (n_items > 0) ALEGO_LAUNCH(mg_copy, dim3(n_items), dim3(MG_T), 0, st, L, pairs, items);
}
void launch_mg_frames(const LmCtx& L, const MgPair* pairs, int n_pairs, int ns_max, hipStream_t st) {
  ALEGO_LAUNCH(mg_frames, dim3((ns_max + 63) / 64, n_pairs), dim3(64), 0, st, L, pairs);
}
void launch_mg_ring(const LmCtx& L, const MgPair* pairs, int n_pairs, int tail_max, hipStream_t st) {
  ALEGO_LAUNCH(mg_ring, dim3(tail_max, n_pairs), dim3(MG_T), 0, st, L, pairs);
}
void launch_mg_move(const LmCtx& L, const MgMove* moves, int n, hipStream_t st) {
  ALEGO_LAUNCH(mg_move, dim3(n), dim3(MG_T), 0, st, L, moves);
}
void launch_mg_retransform(const LmCtx& L, const int* tail, int slot0, int n, int j, hipStream_t st) {
  ALEGO_LAUNCH(mg_retransform, dim3(8, 3, n), dim3(MG_T), 0, st, L, tail, slot0, j);
}
