// kernels_loc.hip — localisation mode (alego_loc_enable): every slot of the handle registers its scans against ONE
// frozen key-frame map instead of its own newest key frames.
//
//   loc_select     one workgroup per slot that maps this scan, behind lm_prepare on the slot's LaserMapping stream: the window of the
//                  frame = the K key frames nearest to the pose transformAssociateToMap has just produced (loc_math.h), written to `rec`
//                  in ascending id order.  LI_REBUILD is raised only when the window differs from the last one, so an unchanged window
//                  costs no rebuild; the host reads nothing back.
// The local map of the window is built by map_update / map_accum (kernels_map.hip) from the store's pre-sorted runs — LmCtx::fr_stride /
// fr_mod tell them where a frame lives — and registered by the unchanged lm_knn / lm_fit / lm_solve.  The store itself is filled once by
// lm_host_loc_enable (lm_host.hip) with lm_store_kf's re-transform path and the key-frame sort jobs the ring uses.
//
//   loc_fill       the same store built (alego_loc_enable_from_map) or rebuilt (alego_loc_update_from_map) from a slot's archive of a mapping
//                  handle without a frame crossing to the host, a chunk of frames per launch
//   loc_reset_windows   after a rebuild: every slot's window is emptied, its next mapping frame selects in the new map
#include <algorithm>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_common.h"
#include "kf_store.h"
#include "loc_math.h"
#include "loc_store.h"
#include "prof.h"
#include "wave.h"

#define LS_T 256
#define LS_KMAX 512   // = MAP_KMAX (kernels_map.hip): alego_create refuses a larger recent_keyframe_num

// grid (slots of the launch)
__global__ void __launch_bounds__(LS_T) loc_select(DevCtx d, LmCtx L) {
  const int slot = blockIdx.x + d.slot0, tid = threadIdx.x;
  int* li = L.li + (size_t)slot * LI_COUNT;
  if (!li[LI_RUN]) return;
  __shared__ int s_win[LS_KMAX], s_w[LS_T / 64], s_diff;
  __shared__ unsigned long long s_min[LS_T / 64];
  double* ld = L.ld + (size_t)slot * LD_COUNT;
  const float px = (float)ld[LD_T_M2L + 0], py = (float)ld[LD_T_M2L + 1], pz = (float)ld[LD_T_M2L + 2];   // :250-252, as lc_detect reads it
  const int n = (loc_finite(px) && loc_finite(py) && loc_finite(pz)) ? L.loc_n : 0;
  const float r2 = L.loc_r2;
  const float* kp = kf_pose_of(L, kf_row_at(L, slot, 0));   // the rows of the map store (frame i < loc_n <= fr_mod is entry i)
  const int K = min(L.K, LS_KMAX);
  int c = 0;
  for (int i = tid; i < n; i += LS_T) c += loc_key(kp + (size_t)i * KF_POSE_W, i, px, py, pz, r2) != ~0ull ? 1 : 0;
  int ncand;
  block_excl_scan<LS_T / 64>(c, s_w, &ncand);
  // more candidates than the window holds: the K-th smallest key, by K rounds of "smallest key above the last one" (keys are unique)
  unsigned long long thr = ~0ull;
  if (ncand > K) {
    unsigned long long last = 0ull;
    for (int r = 0; r < K; ++r) {
      unsigned long long best = ~0ull;
      for (int i = tid; i < n; i += LS_T) {
        const unsigned long long key = loc_key(kp + (size_t)i * KF_POSE_W, i, px, py, pz, r2);
        if (r == 0 || key > last) best = min(best, key);
      }
      last = block_min_u64<LS_T / 64>(best, s_min);
    }
    thr = last;
  }
  // the selected frames in ascending id order
  int nsel = 0;
  for (int i0 = 0; i0 < n; i0 += LS_T) {
    const int i = i0 + tid;
    const unsigned long long key = i < n ? loc_key(kp + (size_t)i * KF_POSE_W, i, px, py, pz, r2) : ~0ull;
    const int sel = (key != ~0ull && key <= thr) ? 1 : 0;
    int tot;
    const int ex = block_excl_scan<LS_T / 64>(sel, s_w, &tot);
    if (sel && nsel + ex < LS_KMAX) s_win[nsel + ex] = i;
    nsel += tot;
  }
  nsel = min(nsel, K);
  int* rec = L.rec + (size_t)slot * L.K;
  const int nprev = li[LI_REC_CNT];
  if (tid == 0) s_diff = nprev != nsel ? 1 : 0;
  __syncthreads();
  for (int j = tid; j < min(nsel, nprev); j += LS_T) if (rec[j] != s_win[j]) s_diff = 1;
  __syncthreads();
  const int diff = s_diff;
  if (diff) for (int j = tid; j < nsel; j += LS_T) rec[j] = s_win[j];
  if (tid == 0) {
    ld[LD_LOC_P + 0] = (double)px; ld[LD_LOC_P + 1] = (double)py; ld[LD_LOC_P + 2] = (double)pz;
    li[LI_REC_CNT] = nsel;
    if (diff) { li[LI_REBUILD] = 1; li[LI_NREBUILD] += 1; }
  }
}

void launch_loc_select(const DevCtx& d, const LmCtx& L, hipStream_t st) {
  ALEGO_LAUNCH(loc_select, dim3(d.n_launch), dim3(LS_T), 0, st, d, L);
}

// ---- the batched build of the map store from a slot's archive of a mapping handle --------------------------------
// loc_fill: grid (point blocks, 3 kinds, frames of the chunk), one point per lane.  Frame f = f0 + blockIdx.z of the source archive S goes
//   * as it is stored (sensor frame) into row f of the store: kf_raw_* / kf_cnt / kf_pose, what frame_to_row writes for a frame of the host;
//   * transformed by its key pose into slot blockIdx.z of the staging area: corner, and surf followed by outlier — what kf_row_to_tmp
//     writes into kf_tmp_* for one frame — for the chunk's sort jobs (VoxelGrid mode 1), whose device words it writes as well.
// The load comes from a clamped index and is issued before the bounds test, so no lane waits for a load behind a branch; counts are
// clamped to the store's capacities and every source index to the source's (the host has refused an oversize frame before the launch).
// No atomics, no wait between workgroups: every output element has one writer.
#define LF_T 256
__global__ void __launch_bounds__(LF_T) loc_fill(LmCtx L, KfArcSrc S, int f0, int n_frames, float4* stage_c, float4* stage_s, int* words) {
  const int j = blockIdx.z, f = f0 + j, kind = blockIdx.y;
  const bool first = blockIdx.x == 0 && kind == KF_CORNER && threadIdx.x == 0;
  int* w = words + (size_t)j * LJ_W;
  if (f >= n_frames) {   // the tail of the last chunk: its jobs are off
    if (first) w[LJ_ENABLE] = 0;
    return;
  }
  const int* tab = kf_src_tab(S, f);
  const int r_c = max(tab[AT_N + KF_CORNER], 0), r_s = max(tab[AT_N + KF_SURF], 0), r_o = max(tab[AT_N + KF_OUTL], 0);
  const int n_c = min(r_c, L.kf_cap_c), n_s = min(r_s, L.kf_cap_s), n_o = min(r_o, L.kf_cap_o);
  const int n = kf_pick(kind, n_c, n_s, n_o);
  const size_t row = kf_row_at(L, 0, f);   // (the store: fr_stride = 0, frame f < fr_mod is entry f)
  if (first) {
    int* cnt = kf_cnt_of(L, row);
    float* kp = kf_pose_of(L, row);
    const float* sp = kf_src_pose(S, f);
    cnt[KF_CORNER] = n_c; cnt[KF_SURF] = n_s; cnt[KF_OUTL] = n_o; cnt[KF_KINDS] = 0;
#pragma unroll
    for (int k = 0; k < KF_POSE_W; ++k) kp[k] = k < 6 ? sp[k] : 0.f;
    w[LJ_N_C] = n_c; w[LJ_N_S] = n_s + n_o; w[LJ_ROW] = f; w[LJ_ENABLE] = 1;
  }
  if ((int)blockIdx.x * LF_T >= n) return;   // (uniform per workgroup)
  float m[3][4];
  keypose_matrix(kf_src_pose(S, f), m);
  const long long off = (long long)tab[AT_OFF] + kf_pick(kind, 0, r_c, r_c + r_s);
  const int i = blockIdx.x * LF_T + threadIdx.x;
  const float4 p = S.pts[kf_src_point(S, off + min(i, n - 1))];
  float4* raw = kf_raw_of(L, row, kind);
  float4* dst = kf_pick(kind, stage_c + (size_t)j * L.kf_cap_c, stage_s + (size_t)j * L.total_cap, stage_s + (size_t)j * L.total_cap + n_s);
  if (i < n) { raw[i] = p; dst[i] = kf_transform(m, p); }
}
static_assert(KF_CNT_W == KF_KINDS + 1 && KF_POSE_W == 8, "loc_fill writes a whole row of kf_cnt / kf_pose");

void launch_loc_fill(const LmCtx& L, const KfArcSrc& S, int f0, int n_frames, int chunk, int n_max, float4* stage_c, float4* stage_s, int* words, hipStream_t st) {
  const int cap = std::max(L.kf_cap_c, std::max(L.kf_cap_s, L.kf_cap_o));
  const int gx = std::max(1, (std::min(std::max(n_max, 0), cap) + LF_T - 1) / LF_T);
  ALEGO_LAUNCH(loc_fill, dim3(gx, KF_KINDS, chunk), dim3(LF_T), 0, st, L, S, f0, n_frames, stage_c, stage_s, words);
}

// kf_reset_window for every slot: the window is emptied, the voxel lists and the local maps are stale; the slot's next mapping frame selects and rebuilds
__global__ void __launch_bounds__(LF_T) loc_reset_windows(LmCtx L, int n_slots) {
  const int s = blockIdx.x * LF_T + threadIdx.x;
  if (s >= n_slots) return;
  int* li = L.li + (size_t)s * LI_COUNT;
  kf_reset_window([&](int w, int v) { li[w] = v; });
}
void launch_loc_reset_windows(const LmCtx& L, int n_slots, hipStream_t st) {
  ALEGO_LAUNCH(loc_reset_windows, dim3((n_slots + LF_T - 1) / LF_T), dim3(LF_T), 0, st, L, n_slots);
}

extern "C" int alego_loc_select(const float* keyposes6, int32_t n, const float xyz[3], double radius, int32_t k, int32_t* ids) {
  if (n < 0 || k < 0 || !xyz || (n > 0 && !keyposes6) || (n > 0 && k > 0 && !ids)) return ALEGO_ERR_ARG;
  if (!loc_finite(xyz[0]) || !loc_finite(xyz[1]) || !loc_finite(xyz[2])) return 0;
  const float r2 = loc_r2(radius);
  std::vector<unsigned long long> keys;
  for (int i = 0; i < n; ++i) {
    const unsigned long long key = loc_key(keyposes6 + (size_t)i * 6, i, xyz[0], xyz[1], xyz[2], r2);
    if (key != ~0ull) keys.push_back(key);
  }
  std::sort(keys.begin(), keys.end());
  if ((int)keys.size() > k) keys.resize(k);
  std::vector<int32_t> sel;
  for (unsigned long long key : keys) sel.push_back((int32_t)(key & 0xffffffffu));
  std::sort(sel.begin(), sel.end());
  for (size_t j = 0; j < sel.size(); ++j) ids[j] = sel[j];
  return (int)sel.size();
}
