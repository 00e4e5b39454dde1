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
#include <algorithm>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_common.h"
#include "kf_store.h"
#include "loc_math.h"
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
