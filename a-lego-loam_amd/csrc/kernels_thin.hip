// kernels_thin.hip — a slot's key-frame archive thinned in place on gfx950 (alego_map_thin).  The rule is thin_math.h's;
// the host (lm_host.hip) reads the counts back once after th_select and knows every size from then on.
//
//   th_select       one wavefront per slot: the greedy pass is sequential over the frames and parallel over the kept set - lane l tests kept
//                   frames l, l + 64, ... and a wave vote decides.  The first TH_LDS_KEPT kept positions live in LDS, the others are read from
//                   the poses.  A workgroup of ONE wavefront: the barrier per frame that publishes lane 0's append costs no wait for another wave.
//                   Writes the old -> new id table (the keep mask), new -> old, the new point offsets, N', P' and the first dropped id.
//   th_gather       the hot path: the points behind the first dropped frame, from their old place to a staging buffer.  A work list of (slot, item of
//                   MG_ITEM destination points); a lane finds its frame by binary search in the new offsets and copies one float4, four in flight.
//                   Source and destination ranges of different workgroups overlap in place, so writing in place is a race: th_scatter copies
//                   the staged range back, 16 B per lane and access, in a launch of its own.  The prefix before the first drop is not touched.
//   th_rows_read    one lane per kept frame behind the first drop: its arc_tab row with the new offset, pose, stamp and - with the graph on - the
//                   chain edge composed over its run of old edges, into the staging rows (a lane writing row m in place while another still
//                   reads row m is the same race).
//   th_rows_write   the staged rows into rows first .. N' - 1; one lane per loop edge remaps its ids in place; lane 0 of a slot moves the counters,
//                   discards the estimate and clears the window as alego_lm_reset_window does.
// The ring rows of the newest min(N', K + 1) frames are refilled by mg_ring (kernels_merge.hip) reading the slot's own archive, followed by
// mg_retransform and the key-frame sort rounds as after a merge.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/alego_mi355x.h"
#include "kf_store.h"
#include "merge_math.h"
#include "prof.h"
#include "thin.h"
#include "thin_math.h"

#define TH_W 64   // th_select's workgroup: one wavefront

static_assert(MG_ITEM == 4 * MG_T, "th_gather / th_scatter: four float4 per lane and item");

// grid (jobs), TH_W threads
__global__ void __launch_bounds__(TH_W) th_select(LmCtx L, ThJob* jobs) {
  const ThJob J = jobs[blockIdx.x];
  __shared__ float sx[TH_LDS_KEPT], sy[TH_LDS_KEPT], sz[TH_LDS_KEPT];
  const int lane = threadIdx.x, n = J.n;
  if (J.slot >= 0) {   // the protect mask of an archive: frame 0, the resident ring, the endpoints of the stored loop edges
    const int ring = min(n, L.KR);
    for (int i = lane; i < n; i += TH_W) J.protect[i] = (i == 0 || i >= n - ring) ? 1 : 0;
    __syncthreads();
    const int nl = L.pg_loops_cap > 0 ? pg_stat_of(L, J.slot)[PS_LOOPS] : 0;
    const alego_graph_edge* lp = L.pg_loops + (size_t)J.slot * L.pg_loops_cap;
    for (int l = lane; l < nl; l += TH_W) {
      const int a = lp[l].from, b = lp[l].to;
      if (a >= 0 && a < n) J.protect[a] = 1;
      if (b >= 0 && b < n) J.protect[b] = 1;
    }
  }
  __syncthreads();
  int nk = 0, pts = 0, first = n, p0 = 0;   // (the same in every lane)
  for (int i = 0; i < n; ++i) {
    const float* ki = J.pose + (size_t)i * J.pose_stride;
    const float k3[3] = {ki[0], ki[1], ki[2]};
    bool drop = false;
    if (!J.protect[i]) {
      for (int base = 0; base < nk && !drop; base += TH_W) {
        const int j = base + lane;
        bool hit = false;
        if (j < nk) {
          float jx, jy, jz;
          if (j < TH_LDS_KEPT) { jx = sx[j]; jy = sy[j]; jz = sz[j]; }
          else { const float* kj = J.pose + (size_t)J.old_id[j] * J.pose_stride; jx = kj[0]; jy = kj[1]; jz = kj[2]; }
          hit = th_suppresses(jx, jy, jz, k3, J.r2);
        }
        drop = __any(hit ? 1 : 0) != 0;
      }
    }
    if (!drop) {
      if (lane == 0) {
        J.new_id[i] = nk; J.old_id[nk] = i; J.new_off[nk] = pts;
        if (nk < TH_LDS_KEPT) { sx[nk] = k3[0]; sy[nk] = k3[1]; sz[nk] = k3[2]; }
      }
      if (J.tab) pts += arc_tab_points(J.tab + (size_t)i * AT_W);
      ++nk;
    } else {
      if (lane == 0) J.new_id[i] = -1;
      if (first == n) { first = i; p0 = pts; }   // (the offset the next kept frame gets: rows and points before it stay)
    }
    __syncthreads();   // lane 0's append is visible to the wavefront's next frame
  }
  if (lane == 0) { J.new_off[nk] = pts; J.cnt[0] = nk; J.cnt[1] = pts; J.cnt[2] = first; J.cnt[3] = p0; }
}

// the archive index a moved destination point comes from: d in [J.p0, J.p_new)
__device__ __forceinline__ int th_source_of(const LmCtx& L, const ThJob& J, int d) {
  int lo = J.first, hi = J.n_new - 1;   // the largest m in [first, N' - 1] with new_off[m] <= d (an empty frame shares its offset with the next)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (J.new_off[mid] <= d) lo = mid; else hi = mid - 1;
  }
  return arc_tab_of(L, J.slot, J.old_id[lo])[AT_OFF] + (d - J.new_off[lo]);
}

// grid (items), MG_T threads.  Every item has at least one point; sources lie inside the slot's stored points, the stage holds p_new - p0 points per job.
__global__ void __launch_bounds__(MG_T) th_gather(LmCtx L, const ThJob* jobs, const int2* items, float4* stage) {
  const int2 it = items[blockIdx.x];
  const ThJob& J = jobs[it.x];
  const float4* src = L.arc_pts + (size_t)J.slot * L.arc_points_cap;
  float4* dst = stage + J.stage_pt;
  const int base = it.y * MG_ITEM + threadIdx.x, n = J.p_new - J.p0;
  // (four unconditional loads at clamped indices, as mg_copy's)
  const float4 v0 = src[th_source_of(L, J, J.p0 + min(base, n - 1))], v1 = src[th_source_of(L, J, J.p0 + min(base + MG_T, n - 1))];
  const float4 v2 = src[th_source_of(L, J, J.p0 + min(base + 2 * MG_T, n - 1))], v3 = src[th_source_of(L, J, J.p0 + min(base + 3 * MG_T, n - 1))];
  if (base < n) dst[base] = v0;
  if (base + MG_T < n) dst[base + MG_T] = v1;
  if (base + 2 * MG_T < n) dst[base + 2 * MG_T] = v2;
  if (base + 3 * MG_T < n) dst[base + 3 * MG_T] = v3;
}

// grid (items), MG_T threads: the staged range back behind the untouched prefix
__global__ void __launch_bounds__(MG_T) th_scatter(LmCtx L, const ThJob* jobs, const int2* items, const float4* stage) {
  const int2 it = items[blockIdx.x];
  const ThJob& J = jobs[it.x];
  const float4* src = stage + J.stage_pt;
  float4* dst = L.arc_pts + (size_t)J.slot * L.arc_points_cap + J.p0;
  const int base = it.y * MG_ITEM + threadIdx.x, n = J.p_new - J.p0;
  const float4 v0 = src[min(base, n - 1)], v1 = src[min(base + MG_T, n - 1)], v2 = src[min(base + 2 * MG_T, n - 1)], v3 = src[min(base + 3 * MG_T, n - 1)];
  if (base < n) dst[base] = v0;
  if (base + MG_T < n) dst[base + MG_T] = v1;
  if (base + 2 * MG_T < n) dst[base + 2 * MG_T] = v2;
  if (base + 3 * MG_T < n) dst[base + 3 * MG_T] = v3;
}

// grid (ceil(rows_max / 64), jobs), 64 threads: lane t of a job stages new row first + t
__global__ void __launch_bounds__(64) th_rows_read(LmCtx L, const ThJob* jobs, ThRow* stage) {
  const ThJob& J = jobs[blockIdx.y];
  const int m = J.first + blockIdx.x * 64 + threadIdx.x;
  if (m >= J.n_new) return;
  const int o = J.old_id[m];
  ThRow r;
  const int* ts = arc_tab_of(L, J.slot, o);
  r.tab[AT_OFF] = J.new_off[m];
#pragma unroll
  for (int k = 0; k < KF_KINDS; ++k) r.tab[AT_N + k] = ts[AT_N + k];
  const float* ps = arc_pose_of(L, J.slot, o);
  for (int k = 0; k < KF_POSE_W; ++k) r.pose[k] = ps[k];
  r.stamp = L.arc_stamp[arc_row(L, J.slot, o)];
  if (L.pg_loops_cap > 0) th_compose_edge(L.pg_chain + arc_row(L, J.slot, 0), J.old_id[m - 1], o, m, &r.e);   // (first >= 1: frame 0 is protected)
  stage[J.stage_row + (m - J.first)] = r;
}

// grid (ceil(lanes_max / 64), jobs), 64 threads
__global__ void __launch_bounds__(64) th_rows_write(LmCtx L, const ThJob* jobs, const ThRow* stage) {
  const ThJob& J = jobs[blockIdx.y];
  const int t = blockIdx.x * 64 + threadIdx.x, m = J.first + t;
  if (m < J.n_new) {
    const ThRow& r = stage[J.stage_row + t];
    int* td = arc_tab_of(L, J.slot, m);
    for (int k = 0; k < AT_W; ++k) td[k] = r.tab[k];
    float* pd = arc_pose_of(L, J.slot, m);
    for (int k = 0; k < KF_POSE_W; ++k) pd[k] = r.pose[k];
    L.arc_stamp[arc_row(L, J.slot, m)] = r.stamp;
    if (L.pg_loops_cap > 0) L.pg_chain[arc_row(L, J.slot, m)] = r.e;
  }
  if (t < J.n_loops) {
    alego_graph_edge* e = L.pg_loops + (size_t)J.slot * L.pg_loops_cap + t;
    alego_graph_edge x;
    if (th_remap_edge(e, J.new_id, J.n, &x)) { e->from = x.from; e->to = x.to; }
  }
  if (t == 0) {
    int* st = arc_stat_of(L, J.slot);
    st[AS_FRAMES] = J.n_new; st[AS_DROPPED] = 0; st[AS_POINTS] = J.p_new;
    int* li = L.li + (size_t)J.slot * LI_COUNT;
    li[LI_NKF] = J.n_new;
    kf_reset_window([&](int w, int v) { li[w] = v; });
    if (L.pg_loops_cap > 0) pg_stat_of(L, J.slot)[PS_EST] = 0;   // the last estimate's pose count no longer matches
  }
}

void launch_th_select(const LmCtx& L, ThJob* jobs, int n_jobs, hipStream_t st) {
  if (n_jobs > 0) ALEGO_LAUNCH(th_select, dim3(n_jobs), dim3(TH_W), 0, st, L, jobs);
}
void launch_th_gather(const LmCtx& L, const ThJob* jobs, const int2* items, int n_items, float4* stage, hipStream_t st) {
  if (n_items > 0) ALEGO_LAUNCH(th_gather, dim3(n_items), dim3(MG_T), 0, st, L, jobs, items, stage);
}
void launch_th_scatter(const LmCtx& L, const ThJob* jobs, const int2* items, int n_items, const float4* stage, hipStream_t st) {
  if (n_items > 0) ALEGO_LAUNCH(th_scatter, dim3(n_items), dim3(MG_T), 0, st, L, jobs, items, stage);
}
void launch_th_rows_read(const LmCtx& L, const ThJob* jobs, int n_jobs, int rows_max, ThRow* stage, hipStream_t st) {
  if (rows_max > 0) ALEGO_LAUNCH(th_rows_read, dim3((rows_max + 63) / 64, n_jobs), dim3(64), 0, st, L, jobs, stage);
}
void launch_th_rows_write(const LmCtx& L, const ThJob* jobs, int n_jobs, int lanes_max, const ThRow* stage, hipStream_t st) {
  ALEGO_LAUNCH(th_rows_write, dim3((std::max(lanes_max, 1) + 63) / 64, n_jobs), dim3(64), 0, st, L, jobs, stage);
}
