// kernels_lm.hip — LaserMapping scan-to-map registration on gfx950
// (replaces src/laserMapping.cpp:154-166,188-192,194-244,315-559 and laserMapping.h:164-194).
//
//   lm_prepare     laserOdomHandler + mainLoop gate + transformAssociateToMap; stages the inputs
//   lm_concat      a19: concatenation of the <= K most recent key frames (already in the map frame)
//   (voxel.h)      a19/a20: VoxelGrid of the map (only when the key-frame set changed) and of the scan
//   lm_total       laser_surf_total_ = laser_surf_ds_ + laser_outlier_ds_ (:337-340); ALEGO_LM_TOTAL_MERGE=0 only
//   lm_total_merge laser_outlier_ds_ of a small /outlier cloud and laser_surf_total_ds_ by merging (:333-342; vox_merge.h)
//   lm_grid_*      uniform grid (cell >= 1 m) over the down-sampled maps: exact 5-NN for every
//                  accepted query because acceptance needs d5^2 < 1.0 (:376,:426) — replaces KdTreeFLANN
//   lm_assoc       a21/a22: 5-NN, 3x3 scatter eigen-decomposition (line) / 5x3 Householder LS (plane)
//   lm_solve       a23/a24: both ceres::Solve calls of :360-478 in one workgroup per stream
//   lm_finish / lm_store_kf  saveKeyFramesAndFactor (no-loop-closure pass-through) + transformUpdate
// The registration guards read "no map yet" as (LI_NKF | LI_REC_CNT) == 0: no key frame in SLAM mode (a window entry implies one), an empty
// window in localisation mode, where LI_NKF stays 0 (kernels_loc.hip).
#include <cstddef>
#include <cstring>

#include "../../include/alego_mi355x.h"
#include "dev_cost.h"
#include "nn_rules.h"
#include "remap_math.h"
#include "prof.h"
#include "kf_store.h"
#include "gmap.h"
#include "vgrid.h"
#include "vox_merge.h"

#define LM_BLOCK 256

DEV_INLINE double* ldp(const LmCtx& L, int slot) { return L.ld + (size_t)slot * LD_COUNT; }
DEV_INLINE int* lip(const LmCtx& L, int slot) { return L.li + (size_t)slot * LI_COUNT; }

// Map sequence = lm_concat, VoxelGrid of the two maps, lm_grid_*, at the start of every mapping frame.  lm_map_update
// (called by lm_prepare's bookkeeping thread) replays the deque bookkeeping of extractSurroundingKeyFrames
// (laserMapping.cpp:206-238) on the list of frame ids and decides whether the local map changed (the reference
// re-assembles and re-filters the identical map on every mapping frame; here only when its content changes):
//   deque not full yet  -> the newest min(n, K) key frames; content changes when a key frame was saved
//   deque full          -> if latest_frame_id_ != n-1: pop front, push frame n-1.  latest_frame_id_ starts at -1, so the
//                          first mapping frame after the deque filled up pushes frame K-1 a second time (and drops
//                          frame 0) although no key frame was saved: the duplicate stays in the window for K-1 further
//                          key frames and doubles that frame's weight in the voxel centroids.  Reproduced as is.
// LI_REBUILD is cleared again by lm_finish at the end of the frame.
DEV_INLINE void lm_map_update(const LmCtx& L, int slot, int* li, int merge) {
  const int nkf = li[LI_NKF];
  if (nkf == 0) return;   // :196-199
  int* rec = L.rec + (size_t)slot * L.K;
  const int cnt = li[LI_REC_CNT];
  bool changed = false;
  if (cnt < L.K) {
    const int nk = min(nkf, L.K);
    changed = li[LI_DIRTY] != 0;
    for (int j = 0; j < nk; ++j) rec[j] = nkf - nk + j;
    li[LI_REC_CNT] = nk;
  } else if (li[LI_LATEST] != nkf - 1) {
    for (int j = 0; j + 1 < L.K; ++j) rec[j] = rec[j + 1];
    rec[L.K - 1] = nkf - 1;
    li[LI_LATEST] = nkf - 1;
    changed = true;
  }
  li[LI_DIRTY] = 0;
  if (changed) { li[LI_REBUILD] = 1; li[LI_NREBUILD] += 1; }
}


// grid (8, 3, slots).  stage: copy /corner_last, /surf_last, /outlier of this scan into the LM inputs.
// stage 0: inputs uploaded by the host (alego_lm_process); 1: copy this scan's clouds and read its odometry from the front end's
// buffers; 2: lm_stage (below) has copied both — LaserMapping runs on its own HIP stream while the front end works on later scans.
__global__ void __launch_bounds__(LM_BLOCK) lm_prepare(DevCtx d, LmCtx L, int stage, int run_hint, int par) {
  const int slot = blockIdx.z + d.slot0, kind = blockIdx.y;
  const int cur = scal_of(d, slot)[SC_CUR];  // LO has completed: features of this scan
  const int sslot = scan_slot_of(d, slot);           // where this scan's features, outliers and odometry hand-over live (its lane, or the slot itself)
  int* li = lip(L, slot);
  if (stage == 1 && run_hint != 0) {   // run_hint == 0: the host knows that no slot of this launch maps this scan (odd frame)
    // (written with unconditional loads + selects: a 3-way if/else chain here was lowered by hipcc 7.2 into
    //  a scalar switch that left the count pointer of the last arm undefined)
    const size_t fb = d.fs_cur >= 0 ? fbuf(d.fs_cur, 0) : fbuf(slot, cur);
    const int n_c = feat_cnt_of(d, fb)[F_LSHARP], n_s = scal_of(d, sslot)[SC_FE_ERR] ? 0 : feat_cnt_of(d, fb)[F_LFLAT], n_o = scal_of(d, sslot)[SC_NOUT];   // (SC_FE_ERR: dev_common.h)
    const float4* src_c = feat_of(d, F_LSHARP, fb);
    const float4* src_s = feat_of(d, F_LFLAT, fb);
    const float4* src_o = d.outlier + (size_t)sslot * d.N;
    const float4* src = kind == 0 ? src_c : (kind == 1 ? src_s : src_o);
    float4* dst = kind == 0 ? L.in_corner + (size_t)slot * L.in_cap_c : (kind == 1 ? L.in_surf + (size_t)slot * L.in_cap_s : L.in_outl + (size_t)slot * L.in_cap_o);
    const int cap = kind == 0 ? L.in_cap_c : (kind == 1 ? L.in_cap_s : L.in_cap_o);
    int n = kind == 0 ? n_c : (kind == 1 ? n_s : n_o);
    if (n > cap) { n = cap; if (threadIdx.x == 0 && blockIdx.x == 0) li[LI_OVERFLOW] = 1; }
    for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < n; i += gridDim.x * LM_BLOCK) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) li[LI_NIN_C + kind] = n;
  }
  if (blockIdx.x != 0 || kind != 0 || threadIdx.x != 0) return;
  double* ld = ldp(L, slot);
  double* po = poses_of(d, sslot);
  const double* pin = stage == 2 ? L.stage_odom + ((size_t)slot * 2 + par) * 8 : po;   // this scan's /odom/lidar
  li[LI_RUN] = 0; li[LI_REBUILD] = 0; li[LI_REBUILD_FB] = 0; li[LI_KF_ADDED] = 0; li[LI_OPTIMIZED] = 0; li[LI_FLAGS] = 0;
  if (stage == 2 ? pin[7] == 0.0 : !scal_of(d, sslot)[SC_ODOM_VALID]) return;  // no /odom/lidar on the initialising scan -> no mapping frame
  // laserOdomHandler :154-166
  for (int k = 0; k < 3; ++k) ld[LD_T_O2L + k] = pin[PO_ODOM_T + k];
  for (int k = 0; k < 4; ++k) ld[LD_Q_O2L + k] = pin[PO_ODOM_Q + k];
  const DQuat qm2o = ldq(ld + LD_Q_M2O), qo2l = ldq(ld + LD_Q_O2L);
  double r[3];
  dq_rotate(qm2o, ld + LD_T_O2L, r);
  for (int k = 0; k < 3; ++k) ld[LD_T_M2L + k] = r[k] + ld[LD_T_M2O + k];
  stq(ld + LD_Q_M2L, dq_mul(qm2o, qo2l));
  for (int k = 0; k < 3; ++k) po[PO_MAP_T + k] = ld[LD_T_M2L + k];   // /odom_aft_mapped
  for (int k = 0; k < 4; ++k) po[PO_MAP_Q + k] = ld[LD_Q_M2L + k];
  // mainLoop gate :107-127
  const int run = (li[LI_FRAME] % d.P.lm_every) == 0;
  li[LI_FRAME] += 1;
  li[LI_RUN] = run;
  if (run_hint >= 0 && run != run_hint) li[LI_OVERFLOW] = 2;  // host launch-skipping logic out of sync
  if (!run) { li[LI_FLAGS] = 8; return; }
  if (L.loc_on) return;   // localisation: the window is loc_select's (kernels_loc.hip), from the pose just associated
  lm_map_update(L, slot, li, d.opt_map_merge);
  li[LI_REBUILD_FB] = li[LI_REBUILD] && !d.opt_map_merge;
}


// grid (8, 3, slots) on the FRONT END's stream: hands this scan over to a LaserMapping that runs on a stream of its own — /odom/lidar
// and its validity into stage_odom[par], and (mapping frames, run_hint != 0) /corner_last, /surf_last, /outlier into the LM inputs.
// After it the front end may overwrite its per-scan buffers; lm_prepare(stage 2) reads only what was staged here.
__global__ void __launch_bounds__(LM_BLOCK) lm_stage(DevCtx d, LmCtx L, int run_hint, int par) {
  const int slot = blockIdx.z + d.slot0, kind = blockIdx.y;
  const int cur = scal_of(d, slot)[SC_CUR];  // LO has completed: features of this scan
  int* li = lip(L, slot);
  if (run_hint != 0) {
    const size_t fb = fbuf(slot, cur);
    const int n_c = feat_cnt_of(d, fb)[F_LSHARP], n_s = scal_of(d, slot)[SC_FE_ERR] ? 0 : feat_cnt_of(d, fb)[F_LFLAT], n_o = scal_of(d, slot)[SC_NOUT];
    const float4* src_c = feat_of(d, F_LSHARP, fb);
    const float4* src_s = feat_of(d, F_LFLAT, fb);
    const float4* src_o = d.outlier + (size_t)slot * d.N;
    const float4* src = kind == 0 ? src_c : (kind == 1 ? src_s : src_o);
    float4* dst = kind == 0 ? L.in_corner + (size_t)slot * L.in_cap_c : (kind == 1 ? L.in_surf + (size_t)slot * L.in_cap_s : L.in_outl + (size_t)slot * L.in_cap_o);
    const int cap = kind == 0 ? L.in_cap_c : (kind == 1 ? L.in_cap_s : L.in_cap_o);
    int n = kind == 0 ? n_c : (kind == 1 ? n_s : n_o);
    if (n > cap) { n = cap; if (threadIdx.x == 0 && blockIdx.x == 0) li[LI_OVERFLOW] = 1; }
    for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < n; i += gridDim.x * LM_BLOCK) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) li[LI_NIN_C + kind] = n;
  }
  if (blockIdx.x != 0 || kind != 0 || threadIdx.x >= 8) return;
  double* so = L.stage_odom + ((size_t)slot * 2 + par) * 8;
  so[threadIdx.x] = threadIdx.x < PO_MAP_T ? poses_of(d, slot)[threadIdx.x] : (scal_of(d, slot)[SC_ODOM_VALID] ? 1.0 : 0.0);
}


// grid (2, K, slots): chronological concatenation of the window's key frames (:238-243), each transformed by its key pose, in
// the reference's order (corner | surf then outlier per frame).  Only the concat + radix-sort VoxelGrid path (ALEGO_MAP_MERGE=0)
// runs it; the default path merges the pre-sorted key frames (kernels_map.hip).
__global__ void __launch_bounds__(LM_BLOCK) lm_concat(DevCtx d, LmCtx L) {
  const int slot = blockIdx.z + d.slot0, j = blockIdx.y;
  int* li = lip(L, slot);
  if (!li[LI_REBUILD_FB]) return;
  const int nk = li[LI_REC_CNT];
  if (j >= nk) return;
  const int* rec = L.rec + (size_t)slot * L.K;
  int offc = 0, offs = 0;
  for (int i = 0; i < j; ++i) { const int* kc = kf_cnt_of(L, kf_row(L, slot, rec[i])); offc += kc[KF_CORNER]; offs += kc[KF_SURF] + kc[KF_OUTL]; }
  const KfRingRow R = kf_ring_row_at(L, slot, kf_entry(L, rec[j]), KF_CORNER);
  const int nc = R.cnt[KF_CORNER], ns = R.cnt[KF_SURF], no = R.cnt[KF_OUTL];
  float m[3][4];
  keypose_matrix(R.pose, m);
  const float4 *sc_ = R.raw, *ss_ = kf_raw_of(L, R.row, KF_SURF), *so_ = kf_raw_of(L, R.row, KF_OUTL);
  float4* dc = L.map_corner_raw + (size_t)slot * L.map_cap_c + offc;
  float4* ds = L.map_surf_raw + (size_t)slot * L.map_cap_s + offs;  // surf then outlier per key frame (:241-242)
  for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < nc; i += gridDim.x * LM_BLOCK) dc[i] = kf_transform(m, sc_[i]);
  for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < ns; i += gridDim.x * LM_BLOCK) ds[i] = kf_transform(m, ss_[i]);
  for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < no; i += gridDim.x * LM_BLOCK) ds[ns + i] = kf_transform(m, so_[i]);
  if (j == nk - 1 && blockIdx.x == 0 && threadIdx.x == 0) { li[LI_KRAW_C] = offc + nc; li[LI_KRAW_S] = offs + ns + no; }
}

// grid (8, slots)
__global__ void __launch_bounds__(LM_BLOCK) lm_total(DevCtx d, LmCtx L) {
  const int slot = blockIdx.y + d.slot0;
  int* li = lip(L, slot);
  if (!li[LI_RUN]) return;
  int ns = li[LI_NCUR_S], no = li[LI_NCUR_O];
  if (ns + no > L.total_cap) { no = L.total_cap - ns; if (threadIdx.x == 0 && blockIdx.x == 0) li[LI_OVERFLOW] = 1; }
  const float4* s = L.cur_surf_ds + (size_t)slot * L.kf_cap_s;
  const float4* o = L.cur_outl_ds + (size_t)slot * L.kf_cap_o;
  float4* t = L.cur_total + (size_t)slot * L.total_cap;
  for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < ns; i += gridDim.x * LM_BLOCK) t[i] = s[i];
  for (int i = blockIdx.x * LM_BLOCK + threadIdx.x; i < no; i += gridDim.x * LM_BLOCK) t[ns + i] = o[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) li[LI_NTOTAL] = ns + no;
}

// ---- lm_total_merge (ALEGO_LM_TOTAL_MERGE, the default): one light workgroup per slot in the place of lm_total, the second VoxelGrid round and, for
// a small /outlier cloud, the first round's outlier job.  The rules are vox_merge.h's.
//   a  /outlier of at most LT_OCAP points: laser_outlier_ds_ = VoxelGrid(lm_leaf_outlier) by rank-by-counting (vox_plan leaves that job out)
//   b  laser_surf_total_ds_ by merging laser_surf_ds_, which round 1 left in voxel-key order, with laser_outlier_ds_
// A slot that vm_refuse turns down gets lm_total's concatenation and puts its round-2 job on the work lists of the group's second VoxelGrid
// context, which vox_plan would have written: one vox_small launch with a small grid stays behind for them.  No __threadfence() here: with one
// workgroup per slot an agent-scope fence each costs the other stream groups' kernels more than the second round did.
#define LT_T 256
#define LT_B 8   // S points a thread has in flight
DEV_INLINE void lt_box_reduce(float mn[3], float mx[3], float (*s_red)[LT_T / 64]) {   // every thread gets the workgroup's box
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();   // the previous readers of s_red are done
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bfly_minmax_f32(mn[a], mx[a]);
    if (lane == 0) { s_red[a][wave] = mn[a]; s_red[3 + a][wave] = mx[a]; }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = s_red[a][0]; mx[a] = s_red[3 + a][0];
#pragma unroll
    for (int w = 1; w < LT_T / 64; ++w) { mn[a] = fminf(mn[a], s_red[a][w]); mx[a] = fmaxf(mx[a], s_red[3 + a][w]); }
  }
}
// s_key[0, n) -> s_skey (the keys in stable order) and s_idx (their input positions); n <= LT_OCAP
DEV_INLINE void lt_order(const vm_u64* s_key, vm_u64* s_skey, unsigned short* s_idx, int n) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += LT_T) { const int r = vm_rank(s_key, n, i); s_skey[r] = s_key[i]; s_idx[r] = (unsigned short)i; }
  __syncthreads();
}

// grid (slots)
__global__ void __launch_bounds__(LT_T) lm_total_merge(DevCtx d, LmCtx L, LtLists W) {
  const int slot = blockIdx.x + d.slot0, tid = threadIdx.x;
  int* li = lip(L, slot);
  __shared__ vm_u64 s_key[LT_OCAP], s_skey[LT_OCAP];
  __shared__ unsigned short s_idx[LT_OCAP];
  __shared__ int s_osb[LT_OCAP];       // part b: an O element between two S keys: owner thread << 16 | S heads of the owner's chunk before it; -1: its key is one of S's
  __shared__ int s_oop[LT_OCAP + 1];   // part b: voxels of O elements alone among the sorted ranks below j
  __shared__ int s_base[LT_T];         // part b: S heads before a thread's chunk
  __shared__ float s_red[6][LT_T / 64];
  __shared__ int s_w[LT_T / 64];
  int state = 0;   // 0: nothing left to do for the slot; 1 / 2: its round-2 job goes on the small / big list
  if (li[LI_RUN]) {
    const float FMAX = 3.402823466e+38f;
    int no = li[LI_NCUR_O];
    // ---- a: the outlier filter (bit for bit what vox_small_job writes)
    const int nin = min(li[LI_NIN_O], L.in_cap_o);
    if (nin <= LT_OCAP) {
      const float4* in = L.in_outl + (size_t)slot * L.in_cap_o;
      float4* out = L.cur_outl_ds + (size_t)slot * L.kf_cap_o;
      const int cap = L.kf_cap_o;
      const float inv = 1.0f / d.P.lm_leaf_outlier;
      int nvox = 0, full = nin;   // full: what the filter produces before the capacity cuts it
      if (nin > 0) {
        float mn[3] = {FMAX, FMAX, FMAX}, mx[3] = {-FMAX, -FMAX, -FMAX};
        for (int i = tid; i < nin; i += LT_T) vgr_box_add(mn, mx, in[i]);
        lt_box_reduce(mn, mx, s_red);
        if (vgr_leaf_too_small(mn, mx, inv)) {   // output = input
          for (int i = tid; i < min(nin, cap); i += LT_T) out[i] = in[i];
        } else {
          const VgrGeom g = vgr_geom(mn, mx, inv);
          for (int i = tid; i < nin; i += LT_T) s_key[i] = vgr_id(g, in[i], inv);   // (u32 ids, wrap included, in the order of their bits)
          lt_order(s_key, s_skey, s_idx, nin);
          for (int t0 = 0; t0 < nin; t0 += LT_T) {
            const int m = t0 + tid;
            const bool head = m < nin && (m == 0 || s_skey[m] != s_skey[m - 1]);
            int tot;
            const int r = nvox + block_excl_scan<LT_T / 64>(head ? 1 : 0, s_w, &tot);
            if (head && r < cap) {
              int b = m + 1;
              while (b < nin && s_skey[b] == s_skey[m]) ++b;
              out[r] = vm_centroid([&](int j) { return in[s_idx[j]]; }, m, b);
            }
            nvox += tot;
          }
          full = nvox;
        }
      }
      no = min(full, cap);
      if (tid == 0) { li[LI_NCUR_O] = no; if (full > cap) li[LI_OVERFLOW] = 1; }
      __syncthreads();   // laser_outlier_ds_ is complete for part b; s_key / s_skey / s_idx are free again
    }
    // ---- b: laser_surf_total_ = laser_surf_ds_ ++ laser_outlier_ds_ (lm_total's truncation), filtered by merging.  The merged cloud itself is never
    // written: nothing reads laser_surf_total_ but the filter.  S's stable-merge position is i + #{O keys < its key} and O's j + #{S keys <= its key}
    // (vox_merge.h), so a voxel's run is an S run followed by the O elements of that key, and its output rank the S heads and the O-only voxels before
    // it.  Every thread owns a contiguous chunk of S and keeps LT_B loads in flight: the kernel is a chain of memory round trips, and the wavefront
    // slots it holds while it waits are what it costs the kernels of the other stream groups.
    const int ns = li[LI_NCUR_S];
    if (ns + no > L.total_cap) { no = L.total_cap - ns; if (tid == 0) li[LI_OVERFLOW] = 1; }
    const int n = ns + no, cap = L.total_cap;
    const float4* S = L.cur_surf_ds + (size_t)slot * L.kf_cap_s;
    const float4* O = L.cur_outl_ds + (size_t)slot * L.kf_cap_o;
    float4* out = L.cur_total_ds + (size_t)slot * L.total_cap;
    const float inv = 1.0f / d.P.lm_leaf_surf;
    const int c = (ns + LT_T - 1) / LT_T, c0 = min(ns, tid * c), c1 = min(ns, c0 + c);   // this thread's S elements
    bool refuse = no > LT_OCAP;
    int heads = 0;   // S elements of the chunk that start a voxel
    if (!refuse && n > 0) {
      float mn[3] = {FMAX, FMAX, FMAX}, mx[3] = {-FMAX, -FMAX, -FMAX};
      int good = 1;   // finite, and S in key order
      for (int j = tid; j < no; j += LT_T) { const float4 p = O[j]; vgr_box_add(mn, mx, p); good &= vm_finite(p); s_key[j] = vkey_of(p, inv); s_osb[j] = -1; }
      lt_order(s_key, s_skey, s_idx, no);
      // S, first pass: box, order, voxel heads, and the O elements that fall strictly between two S keys (s_osb: thread << 16 | its heads before them)
      vm_u64 kprev = 0;
      int ole_prev = 0;   // #{O keys <= the previous S key}
      if (c0 > 0 && c0 < c1) { kprev = vkey_of(S[c0 - 1], inv); ole_prev = vm_count_le(s_skey, no, kprev); }
      for (int b0 = c0; b0 < c1; b0 += LT_B) {
        float4 p[LT_B];
#pragma unroll
        for (int k = 0; k < LT_B; ++k) p[k] = S[min(b0 + k, c1 - 1)];
#pragma unroll
        for (int k = 0; k < LT_B; ++k) {
          const int i = b0 + k;
          if (i < c1) {
            vgr_box_add(mn, mx, p[k]);
            const vm_u64 key = vkey_of(p[k], inv);
            good &= vm_finite(p[k]) && (i == 0 || kprev <= key);
            const int ol = vm_count_less(s_skey, no, key);
            for (int j = ole_prev; j < ol; ++j) s_osb[j] = tid << 16 | heads;
            heads += (i == 0 || kprev != key) ? 1 : 0;
            kprev = key; ole_prev = vm_count_le(s_skey, no, key);
          }
        }
      }
      if ((c0 < c1 && c1 == ns) || (ns == 0 && tid == 0)) for (int j = ole_prev; j < no; ++j) s_osb[j] = tid << 16 | heads;   // behind the last S key
      lt_box_reduce(mn, mx, s_red);
      good = __syncthreads_and(good);
      refuse = vm_refuse(good != 0, no, mn, mx, inv);
    }
    if (!refuse) {
      int nsh;
      const int base = block_excl_scan<LT_T / 64>(heads, s_w, &nsh);   // S heads before the chunk
      s_base[tid] = base;
      int noo = 0;   // voxels that hold O elements only
      for (int t0 = 0; t0 < no; t0 += LT_T) {
        const int j = t0 + tid;
        const bool oh = j < no && s_osb[j] >= 0 && (j == 0 || s_skey[j - 1] != s_skey[j]);
        int tot;
        const int e = noo + block_excl_scan<LT_T / 64>(oh ? 1 : 0, s_w, &tot);
        if (j < no) s_oop[j] = e;
        noo += tot;
      }
      if (tid == 0) s_oop[no] = noo;
      __syncthreads();
      // S, second pass: a head adds its S run (one element, unless a centroid left its voxel into an occupied one), then the O elements of its key
      vm_u64 kprev = c0 > 0 && c0 < c1 ? vkey_of(S[c0 - 1], inv) : 0;
      int hl = 0;
      for (int b0 = c0; b0 < c1; b0 += LT_B) {
        float4 p[LT_B + 1];
#pragma unroll
        for (int k = 0; k <= LT_B; ++k) p[k] = S[min(b0 + k, ns - 1)];   // (one past the chunk: the key behind its last element)
#pragma unroll
        for (int k = 0; k < LT_B; ++k) {
          const int i = b0 + k;
          if (i < c1) {
            const vm_u64 key = vkey_of(p[k], inv);
            if (i == 0 || kprev != key) {
              const int ol = vm_count_less(s_skey, no, key), ole = vm_count_le(s_skey, no, key);
              const int r = base + hl + s_oop[ol];
              ++hl;
              if (r < cap) {
                int nsr = 1;
                if (i + 1 < ns && vkey_of(p[k + 1], inv) == key) while (i + nsr < ns && vkey_of(S[i + nsr], inv) == key) ++nsr;
                out[r] = vm_centroid([&](int q) { return q == 0 ? p[k] : (q < nsr ? S[i + q] : O[s_idx[ol + q - nsr]]); }, 0, nsr + ole - ol);
              }
            }
            kprev = key;
          }
        }
      }
      for (int j = tid; j < no; j += LT_T) {   // the voxels of O elements alone
        if (s_osb[j] >= 0 && (j == 0 || s_skey[j - 1] != s_skey[j])) {
          const int r = s_base[s_osb[j] >> 16] + (s_osb[j] & 0xFFFF) + s_oop[j];
          if (r < cap) {
            int e = j + 1;
            while (e < no && s_skey[e] == s_skey[j]) ++e;
            out[r] = vm_centroid([&](int q) { return O[s_idx[q]]; }, j, e);
          }
        }
      }
      const int nvox = nsh + noo;
      if (tid == 0) { li[LI_NTOTAL] = n; li[LI_NTOTAL_DS] = min(nvox, cap); if (nvox > cap) li[LI_OVERFLOW] = 1; li[LI_TM_FAST] += 1; }
    } else {
      float4* t = L.cur_total + (size_t)slot * L.total_cap;
      for (int i = tid; i < ns; i += LT_T) t[i] = S[i];
      for (int i = tid; i < no; i += LT_T) t[ns + i] = O[i];
      if (tid == 0) { li[LI_NTOTAL] = n; li[LI_TM_LIST] += 1; }
      state = n > W.small_max ? 2 : 1;
    }
  }
  // ---- the work lists of the round-2 context (vox_plan's part): a refused slot appends its job.  No fence and no last workgroup: the counters of this
  // launch were zeroed by the launch before it (two sets, alternating), and the end of the kernel publishes lists and counters to vox_small.
  if (tid == 0) {
    if (state == 1) W.list_small[atomicAdd(&W.cnt[0], 1)] = slot - L.vox_slot0;   // (the context has one job per slot of the stream group)
    else if (state == 2) W.list_big[atomicAdd(&W.cnt[1], 1)] = slot - L.vox_slot0;
    if (blockIdx.x == 0) { W.cnt_next[0] = 0; W.cnt_next[1] = 0; }
  }
}

// the cell of a point in the grid g of nn_rules.h's exact lattice (nn_lm_coord): its coordinates relative to the grid's origin cell and its clamped index
DEV_INLINE int grid_cell(const GridGeom& g, float x, float y, float z, int* cx, int* cy, int* cz) {
  *cx = nn_lm_coord(x, g.inv) - g.ox; *cy = nn_lm_coord(y, g.inv) - g.oy; *cz = nn_lm_coord(z, g.inv) - g.oz;
  return nn_lm_index(*cx, *cy, *cz, g.gx, g.gy, g.gz);
}

// grid (2, slots): the whole uniform-grid build of one map by one workgroup — geometry from the VoxelGrid bounding box, cell
// counts, exclusive scan, cell-sorted copy.  Only the streams whose map was rebuilt this frame do anything (≈1 in 16), and
// a filtered map is a few thousand points: four launches (setup, count, scan, fill) cost more in launch latency than in work.
__global__ void __launch_bounds__(LM_BLOCK) lm_grid_build(DevCtx d, LmCtx L) {
  const int slot = blockIdx.y + d.slot0, m = blockIdx.x;
  const int* li = lip(L, slot);
  if (!li[LI_REBUILD]) return;
  __shared__ GridGeom s_g;
  __shared__ int s[LM_BLOCK / 64];
  __shared__ int s_run;
  if (threadIdx.x == 0) {
    const unsigned* bb = d.opt_map_merge ? L.map_bbox + ((size_t)slot * 2 + m) * 8 : L.vox_bbox + ((size_t)(slot - L.vox_slot0) * 2 + m) * 8;
    GridGeom g;
    float mn[3], mx[3];
    vgr_box_load(bb, mn, mx);
    if (li[LI_KRAW_C + m] <= 0) { for (int a = 0; a < 3; ++a) { mn[a] = 0.f; mx[a] = 0.f; } }
    float cell = nn_lm_cell(d.P.knn_max_dist);   // cell^2 >= knn_max_dist: the 27 cells around a query hold every candidate lm_knn keeps (nn_rules.h)
    // the box is the RAW window's: an f32 voxel centroid can lie an ulp outside it, so one cell of margin on either side keeps every map point
    // unclamped in its true cell
    int lo[3], hi[3];
    for (;;) {
      for (int a = 0; a < 3; ++a) { lo[a] = nn_lm_coord(mn[a], 1.0f / cell) - 1; hi[a] = nn_lm_coord(mx[a], 1.0f / cell) + 1; }
      const long long ex = (long long)hi[0] - lo[0] + 1, ey = (long long)hi[1] - lo[1] + 1, ez = (long long)hi[2] - lo[2] + 1;
      if (ex <= L.gcap && ey <= L.gcap && ez <= L.gcap && ex * ey * ez <= (long long)L.gcap) { g.gx = (int)ex; g.gy = (int)ey; g.gz = (int)ez; break; }
      cell *= 2.0f;
    }
    g.ox = lo[0]; g.oy = lo[1]; g.oz = lo[2]; g.inv = 1.0f / cell; g.ncell = g.gx * g.gy * g.gz;
    s_g = g;
    L.grid[(size_t)slot * 2 + m] = g;
    s_run = 0;
  }
  __syncthreads();
  const GridGeom g = s_g;
  const int ncell = g.ncell;
  int* cs = L.cell_start + ((size_t)slot * 2 + m) * (L.gcap + 1);
  int* cc = L.cell_cur + ((size_t)slot * 2 + m) * (L.gcap + 1);
  for (int c = threadIdx.x; c <= ncell; c += LM_BLOCK) cs[c] = 0;
  __threadfence_block();
  __syncthreads();
  const int n = li[LI_KDS_C + m];
  const float4* pts = (m == 0 ? L.map_corner_ds + (size_t)slot * L.map_cap_c : L.map_surf_ds + (size_t)slot * L.map_cap_s);
  float4* cp = L.cell_pts + ((size_t)slot * 2 + m) * L.map_cap_s;
  for (int i = threadIdx.x; i < n; i += LM_BLOCK) {
    const float4 p = pts[i];
    int cx, cy, cz;
    atomicAdd(&cs[grid_cell(g, p.x, p.y, p.z, &cx, &cy, &cz)], 1);
  }
  __threadfence_block();
  __syncthreads();
  // exclusive scan of the cell counts (in place) + fill cursors
  for (int c0 = 0; c0 <= ncell; c0 += LM_BLOCK) {
    const int c = c0 + threadIdx.x;
    // (the counts were accumulated by L2 atomics: read them past the CU's vector cache)
    const int v = __hip_atomic_load(&cs[min(c, ncell)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * (c < ncell ? 1 : 0);
    int tot;
    const int ex = block_excl_scan<LM_BLOCK / 64>(v, s, &tot);
    const int run = s_run;
    if (c <= ncell) { const int e2 = run + ex; cs[c] = e2; cc[c] = e2; }
    __syncthreads();
    if (threadIdx.x == 0) s_run = run + tot;   // (read after the next call's barriers)
  }
  __threadfence_block();
  __syncthreads();
  // cell-sorted copy: one contiguous read per cell run in lm_knn (the order inside a cell is whatever the atomics give:
  // the k-NN result does not depend on it, ties are broken by the point index)
  for (int i = threadIdx.x; i < n; i += LM_BLOCK) {
    const float4 p = pts[i];
    int cx, cy, cz;
    const int pos = atomicAdd(&cc[grid_cell(g, p.x, p.y, p.z, &cx, &cy, &cz)], 1);
    cp[pos] = make_float4(p.x, p.y, p.z, __int_as_float(i));
  }
}

// ---- small dense linear algebra in registers ------------------------------------------
// symmetric 3x3 eigen-decomposition, cyclic Jacobi (same algorithm as the oracle's eig3)
DEV_INLINE void d_eig3(const double Ain[9], double lam[3], double vmax[3], double* lam_mid) {
  double A[9], V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { A[i] = Ain[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
    if (off < 1e-300) break;
    // converged to working precision (round 4, oracle and device alike): the off-diagonal mass is below 1e-40 of the diagonal's, a further rotation moves no entry
    // by more than 1e-20 of the largest.  The absolute test alone ran 8-9 sweeps where 5 suffice — lm_fit was 40 % shorter for it, the bench + 2.8 %.
    if (off <= 1e-40 * (A[0] * A[0] + A[4] * A[4] + A[8] * A[8])) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[p * 3 + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * 3 + q] - A[p * 3 + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double akp = A[k * 3 + p], akq = A[k * 3 + q]; A[k * 3 + p] = c * akp - s * akq; A[k * 3 + q] = s * akp + c * akq; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double apk = A[p * 3 + k], aqk = A[q * 3 + k]; A[p * 3 + k] = c * apk - s * aqk; A[q * 3 + k] = s * apk + c * aqk; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double vkp = V[k * 3 + p], vkq = V[k * 3 + q]; V[k * 3 + p] = c * vkp - s * vkq; V[k * 3 + q] = s * vkp + c * vkq; }
      }
  }
  const double dd[3] = {A[0], A[4], A[8]};
  int imax = 0, imin = 0;
  // ascending order with std::sort-like tie handling on indices (first minimum, last maximum not needed: ties are measure-zero)
  if (dd[1] > dd[imax]) imax = 1;
  if (dd[2] > dd[imax]) imax = 2;
  if (dd[1] < dd[imin]) imin = 1;
  if (dd[2] < dd[imin]) imin = 2;
  int imid = 3 - imax - imin;
  if (imax == imin) { imax = 2; imin = 0; imid = 1; }
  lam[0] = dd[imin]; lam[1] = dd[imid]; lam[2] = dd[imax];
  *lam_mid = dd[imid];
  vmax[0] = V[0 * 3 + imax]; vmax[1] = V[1 * 3 + imax]; vmax[2] = V[2 * 3 + imax];
}

// Eigen::ColPivHouseholderQR<Matrix<double, 5, 3>>::compute() + solve() (laserMapping.cpp:435) — the parity checker's colpiv_qr_solve (where the algorithm's
// source in Eigen 3.3 is cited step by step) specialised to 5 x 3 with everything in registers: the column of largest remaining norm is swapped into place (selects
// over static indices, no indexed register access), Householder reflector (beta, essential, tau) as Householder.h builds it, LAPACK's norm down-date, nonzeroPivots()
// by Eigen's threshold, and the components past it ZERO — a collinear / coincident neighbourhood gets a finite basic solution instead of a division by a ~1e-17 pivot.
// Same operations in the same order as the oracle, fp64, -ffp-contract=off.  A[c][i] = column c, row i (overwritten).
DEV_INLINE void d_colpiv_qr53(double A[3][5], const double b[5], double x[3]) {
  const double eps = 2.220446049250313e-16, tiny = 2.2250738585072014e-308;
  double nu[3], nd[3], hc[3], c[5];
  int perm[3] = {0, 1, 2};
  double maxn = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double s2 = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) s2 += A[k][i] * A[k][i];
    nd[k] = nu[k] = sqrt(s2);
    if (nu[k] > maxn) maxn = nu[k];
  }
  const double threshold_helper = (maxn * eps) * (maxn * eps) / 5.0;
  const double downdate_threshold = 1.4901161193847656e-08;   // sqrt(eps), exact
  int nonzero = 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int big = k;
    double nbig = nu[k];
#pragma unroll
    for (int j = k + 1; j < 3; ++j) if (nu[j] > nbig) { big = j; nbig = nu[j]; }   // maxCoeff: the first of equal maxima
    if (nonzero == 3 && nbig * nbig < threshold_helper * (double)(5 - k)) nonzero = k;
#pragma unroll
    for (int j = k + 1; j < 3; ++j)
      if (big == j) {
#pragma unroll
        for (int i = 0; i < 5; ++i) { const double t = A[k][i]; A[k][i] = A[j][i]; A[j][i] = t; }
        { const double t = nu[k]; nu[k] = nu[j]; nu[j] = t; }
        { const double t = nd[k]; nd[k] = nd[j]; nd[j] = t; }
        { const int t = perm[k]; perm[k] = perm[j]; perm[j] = t; }   // (transposition k of the sequence applied on the right: the oracle's perm after all swaps)
      }
    double tail2 = 0;
#pragma unroll
    for (int i = k + 1; i < 5; ++i) tail2 += A[k][i] * A[k][i];
    const double c0 = A[k][k];
    double beta, tau;
    if (tail2 <= tiny) {
      tau = 0; beta = c0;
#pragma unroll
      for (int i = k + 1; i < 5; ++i) A[k][i] = 0;
    } else {
      beta = sqrt(c0 * c0 + tail2);
      if (c0 >= 0) beta = -beta;
#pragma unroll
      for (int i = k + 1; i < 5; ++i) A[k][i] = A[k][i] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    hc[k] = tau;
    A[k][k] = beta;
    if (tau != 0) {
#pragma unroll
      for (int j = k + 1; j < 3; ++j) {
        double t = 0;
#pragma unroll
        for (int i = k + 1; i < 5; ++i) t += A[k][i] * A[j][i];
        t += A[j][k];
        A[j][k] -= tau * t;
#pragma unroll
        for (int i = k + 1; i < 5; ++i) A[j][i] -= tau * A[k][i] * t;
      }
    }
#pragma unroll
    for (int j = k + 1; j < 3; ++j) {
      if (nu[j] != 0) {
        double t = fabs(A[j][k]) / nu[j];
        t = (1.0 + t) * (1.0 - t);
        t = t < 0 ? 0 : t;
        const double q = nu[j] / nd[j];
        const double t2 = t * (q * q);
        if (t2 <= downdate_threshold) {
          double s2 = 0;
#pragma unroll
          for (int i = k + 1; i < 5; ++i) s2 += A[j][i] * A[j][i];
          nd[j] = nu[j] = sqrt(s2);
        } else nu[j] *= sqrt(t);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) c[i] = b[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double tau = hc[k];
    if (k < nonzero && tau != 0) {
      double t = 0;
#pragma unroll
      for (int i = k + 1; i < 5; ++i) t += A[k][i] * c[i];
      t += c[k];
      c[k] -= tau * t;
#pragma unroll
      for (int i = k + 1; i < 5; ++i) c[i] -= tau * A[k][i] * t;
    }
  }
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    if (k < nonzero) {
      double sum = c[k];
#pragma unroll
      for (int j = k + 1; j < 3; ++j) if (j < nonzero) sum -= A[j][k] * c[j];
      c[k] = sum / A[k][k];
    } else c[k] = 0.0;
  }
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) if (perm[i] == o) v = c[i];
    x[o] = v;
  }
}

// lanes per query of lm_knn: its private sets are merged by group_min_u64<LM_KNN_LANES> (wave.h)
#ifndef LM_KNN_LANES
#define LM_KNN_LANES 4   // measured at 1024 streams: 16 lanes 1008 us, 8: 689, 4: 581, 2: 662, 1: 1176
#endif

// The queries [qlo, qhi) of `kind` that this rank registers: all of them, or — one registration sharded over the ranks of a communicator
// (alego_dist_init) — this rank's contiguous slice of laser_corner_ds_ ++ laser_surf_total_ds_.
DEV_INLINE void lm_shard_slice(const LmCtx& L, int nqc, int nqs, int kind, int* qlo, int* qhi) {
  int lo = 0, hi = nqc + nqs;
  if (L.shard_world > 1) {
    const long long T = nqc + nqs;
    lo = (int)(T * L.shard_rank / L.shard_world); hi = (int)(T * (L.shard_rank + 1) / L.shard_world);
  }
  if (kind == 0) { *qlo = min(lo, nqc); *qhi = min(hi, nqc); } else { *qlo = max(lo - nqc, 0); *qhi = max(hi - nqc, 0); }
}

// Workgroup order of the registration kernels (lm_knn, lm_fit): a 1-D grid of n_launch x (2 kinds x GX) workgroups in which the workgroups of EIGHT
// slots are interleaved — b % 8 picks the slot of the octet, so all workgroups of a slot land on one XCD (workgroup b runs on XCD b mod 8) as before —
// and the octets follow one another: a slot's ~100 workgroups are dispatched back to back instead of one in every n_launch, and its map (2 x 190 KB
// of cell-sorted points) is read into that XCD's L2 once instead of being evicted between them (lm_knn fetched 3x the maps' size from HBM).
DEV_INLINE bool lm_reg_block(const DevCtx& d, int GX, int* slot, int* kind, int* bx) {
  const int per = 2 * GX, b = blockIdx.x, oct = b / (8 * per), r = b - oct * 8 * per;
  const int s = oct * 8 + (r & 7), w = r >> 3;
  *slot = s + d.slot0; *kind = w / GX; *bx = w - (w / GX) * GX;
  return s < d.n_launch;
}
static inline int lm_reg_grid(const DevCtx& d, int GX) { return ((d.n_launch + 7) / 8) * 8 * 2 * GX; }

// 1-D grid (lm_reg_grid): LM_KNN_LANES lanes per query, 128-thread workgroups, LM_ASSOC_GX of them per stream and kind, grid-stride over the queries.
// The lanes of a group split the candidates of the 27 surrounding cells, keep a private top-5 each and merge them
// with five group-wide arg-min rounds.  The kernel is instruction-issue bound: with 4 lanes per query the per-query
// fixed work (pose transform, cell addressing, merge) is shared by 16 queries per wavefront.
#define LM_ASSOC_GX 64
#ifndef LM_KNN_PK
#define LM_KNN_PK 1
#endif
__global__ void __launch_bounds__(128) lm_knn(DevCtx d, LmCtx L) {
  // 1-D grid, lm_reg_block: all workgroups of a stream share one XCD and its L2 and are dispatched back to back (measured HBM traffic of the kernel:
  // 0.60 -> 0.20 MB per scan; throughput unchanged)
  int slot, kind, bx;
  if (!lm_reg_block(d, LM_ASSOC_GX, &slot, &kind, &bx)) return;
  const int gx = LM_ASSOC_GX;
  const int* li = lip(L, slot);
  if (!li[LI_RUN]) return;
  const alego_params& P = d.P;
  if (lm_reg_skipped(li, P)) return;
  const int nq = kind == 0 ? li[LI_NCUR_C] : li[LI_NTOTAL_DS];
  int qlo, qhi;
  lm_shard_slice(L, li[LI_NCUR_C], li[LI_NTOTAL_DS], kind, &qlo, &qhi);
  const float4* qp = kind == 0 ? L.cur_corner_ds + (size_t)slot * L.kf_cap_c : L.cur_total_ds + (size_t)slot * L.total_cap;
  const int nmap = li[LI_KDS_C + kind];
  const GridGeom g = L.grid[(size_t)slot * 2 + kind];
  const int* cs = L.cell_start + ((size_t)slot * 2 + kind) * (L.gcap + 1);
  const float4* cp = L.cell_pts + ((size_t)slot * 2 + kind) * L.map_cap_s;
  const double* ld = ldp(L, slot);
  const DQuat qm = ldq(ld + LD_Q_M2L);
  constexpr int QPB = 128 / LM_KNN_LANES;
  const int sub = threadIdx.x & (LM_KNN_LANES - 1);
  const uint32_t limbits = nn_lm_limit_bits(P.knn_max_dist);   // farther candidates are part of no accepted row: they need not enter the top-5 sets
  // every lane of a wavefront runs the same number of iterations (DPP reads neighbours' registers): clamp, don't exit
  const int nq_round = (nq + QPB - 1) / QPB * QPB;
  for (int qq = bx * QPB + threadIdx.x / LM_KNN_LANES; qq < nq_round; qq += gx * QPB) {
  const int q = min(qq, nq - 1);
  const float4 pin = qp[q];
  // pointAssociateToMap laserMapping.h:187-194 (pose predicted from odometry)
  const double vin[3] = {pin.x, pin.y, pin.z};
  double r[3];
  dq_rotate(qm, vin, r);
  const float sx = (float)(r[0] + ld[LD_T_M2L + 0]), sy = (float)(r[1] + ld[LD_T_M2L + 1]), sz = (float)(r[2] + ld[LD_T_M2L + 2]);
  // exact 5-NN among all points with d^2 < knn_max_dist: they all lie in the 27 surrounding cells (lm_grid_build: cell^2 >= knn_max_dist, exact cell coordinates).
  // A lane's five best candidates are an UNSORTED set of nn_key(distance, map index) with the set's maximum tracked next to it: a candidate that beats the maximum
  // replaces it (five compare-selects) and the maximum is recomputed (four), instead of a five-step insertion sort — the kernel is
  // VALU-bound and the insertion ran for every candidate of every lane (any lane of the wavefront inserting makes all of them pay).
  typedef nn_key_t u64k;
  const u64k KNONE = NN_NONE;
  u64k k0 = KNONE, k1 = KNONE, k2 = KNONE, k3 = KNONE, k4 = KNONE, kmax = KNONE;
  if (nmap >= 5 && q >= qlo && q < qhi) {   // (another rank's query: nothing to search, the row stays empty)
    int cx, cy, cz;
    grid_cell(g, sx, sy, sz, &cx, &cy, &cz);
    // bounds of the nine x-runs of cells first (18 independent loads), then the candidates two per lane at a time
    int rs[9], re[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const int z = cz + r / 3 - 1, y = cy + r % 3 - 1;
      const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.gx - 1);
      const bool in = z >= 0 && z < g.gz && y >= 0 && y < g.gy && x0 <= x1;
      const int c0 = x0 + g.gx * (y + g.gy * z), c1 = x1 + g.gx * (y + g.gy * z);
      // (clamped addresses, not `in ? cs[c0] : 0`: behind a branch every one of the 18 loads waited for the previous one)
      const int a0 = cs[in ? c0 : 0], a1 = cs[in ? c1 + 1 : 0];
      rs[r] = in ? a0 : 0;
      re[r] = in ? a1 : 0;
    }
    const nn_v2f sxy = {sx, sy};   // (x, y) as one packed pair: nn_d2_pk, the same bits as nn_d2
    auto consider = [&](const float4& a) {
#if LM_KNN_PK
      const float dist = nn_d2_pk(sxy, sz, nn_v2f{a.x, a.y}, a.z);
#else
      const float dist = nn_d2(sx, sy, sz, a.x, a.y, a.z);
#endif
      const u64k key = nn_key(dist, (uint32_t)__float_as_int(a.w));
      if (key < kmax && nn_lm_within(dist, limbits)) {
        // (a set that is not full yet holds KNONE entries, which are its maximum; equal KNONE entries are all "the maximum": only one may be replaced)
        const bool e0 = k0 == kmax, e1 = !e0 && k1 == kmax, e2 = !e0 && !e1 && k2 == kmax, e3 = !e0 && !e1 && !e2 && k3 == kmax, e4 = !e0 && !e1 && !e2 && !e3;
        k0 = e0 ? key : k0; k1 = e1 ? key : k1; k2 = e2 ? key : k2; k3 = e3 ? key : k3; k4 = e4 ? key : k4;
        const u64k m01 = k0 > k1 ? k0 : k1, m23 = k2 > k3 ? k2 : k3, m03 = m01 > m23 ? m01 : m23;
        kmax = m03 > k4 ? m03 : k4;
      }
    };
    // the first candidate of each of the nine runs: nine independent loads (a run is usually exhausted by one or two turns)
    float4 first[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) first[r] = cp[rs[r] + sub < re[r] ? rs[r] + sub : 0];
    // the query's own row of cells first, then the rows that share a face with it, the four diagonal ones last: the sets' maxima fall early and
    // fewer of the later candidates enter a set at all (the result does not depend on the order: a set of unique keys)
#ifndef LM_KNN_ORDER
#define LM_KNN_ORDER 1
#endif
    constexpr int ord[9] = {4, 1, 3, 5, 7, 0, 2, 6, 8};
#pragma unroll
    for (int k = 0; k < 9; ++k) { const int r = LM_KNN_ORDER ? ord[k] : k; if (rs[r] + sub < re[r]) consider(first[r]); }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int r = LM_KNN_ORDER ? ord[k] : k;
      for (int t = rs[r] + sub + LM_KNN_LANES; t < re[r]; t += 2 * LM_KNN_LANES) {  // an x-run of cells is contiguous in the cell-sorted copy
        const int t1 = t + LM_KNN_LANES;
        const float4 a0 = cp[t], a1 = cp[t1 < re[r] ? t1 : t];
        consider(a0);
        if (t1 < re[r]) consider(a1);
      }
    }
  }
  // merge the private sets of the query's lanes: five rounds of "smallest key of the group"; the lane that holds it drops it
  float bd[5];
  int bi[5];
  {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const u64k m01 = k0 < k1 ? k0 : k1, m23 = k2 < k3 ? k2 : k3, m03 = m01 < m23 ? m01 : m23, mine = m03 < k4 ? m03 : k4;
      const u64k m = group_min_u64<LM_KNN_LANES>(mine);
      bd[k] = nn_key_d2(m); bi[k] = nn_key_index(m);   // (KNONE: distance bits 0xFFFFFFFF = NaN, index -1 — see `ok` below)
      if (mine == m && m != KNONE) {   // keys are unique (one per map point): exactly one lane of the group, exactly one of its entries
        k0 = k0 == m ? KNONE : k0; k1 = k1 == m ? KNONE : k1; k2 = k2 == m ? KNONE : k2; k3 = k3 == m ? KNONE : k3; k4 = k4 == m ? KNONE : k4;
      }
    }
  }
  // neighbour indices (ascending distance) for lm_fit; idx[0] < 0 = rejected (:376,:426)
  if (sub == 0 && qq < nq) {
    int* kn = lm_knn_of(L, slot, kind, q);
    const bool ok = nn_lm_row_ok(bi[4], bd[4], P.knn_max_dist) && q >= qlo && q < qhi;   // (queries of other ranks' slices give no row here)
#pragma unroll
    for (int k = 0; k < 5; ++k) kn[k] = ok ? bi[k] : -1;
  }
  }
}

// grid (ceil(qcap/128), 2, slots): one thread per query: 3x3 scatter eigen-decomposition (line) or 5x3 Householder
// least squares (plane) on the five neighbours found by lm_knn
#define LM_FIT_GX 20   // x 128 threads: the 1-2 k queries of a kind in one sweep; larger clouds grid-stride
__global__ void __launch_bounds__(128) lm_fit(DevCtx d, LmCtx L) {
  int slot, kind, bx;
  if (!lm_reg_block(d, LM_FIT_GX, &slot, &kind, &bx)) return;   // (workgroup order: see lm_knn)
  const int gx = LM_FIT_GX;
  const int* li = lip(L, slot);
  if (!li[LI_RUN]) return;
  const alego_params& P = d.P;
  if (lm_reg_skipped(li, P)) return;
  const int nq = kind == 0 ? li[LI_NCUR_C] : li[LI_NTOTAL_DS];
  const float4* mp = kind == 0 ? L.map_corner_ds + (size_t)slot * L.map_cap_c : L.map_surf_ds + (size_t)slot * L.map_cap_s;
  for (int q = bx * 128 + threadIdx.x; q < nq; q += gx * 128) {
  const int* kn = lm_knn_of(L, slot, kind, q);
  double* blk = lm_blocks_of(L, slot) + lm_row_of(kind, q, L.kf_cap_c) * LMB_W;
  int bi[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) bi[k] = kn[k];
  lmb_put_none(blk);
  do {
    if (bi[0] < 0) break;
  if (kind == 0) {  // :378-411
    double near[5][3], center[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const float4 m = mp[bi[j]];
      near[j][0] = m.x; near[j][1] = m.y; near[j][2] = m.z;
#pragma unroll
      for (int a = 0; a < 3; ++a) center[a] = center[a] + near[j][a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) center[a] = center[a] / 5.0;
    double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const double zm[3] = {near[j][0] - center[0], near[j][1] - center[1], near[j][2] - center[2]};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) cov[a * 3 + b] = cov[a * 3 + b] + zm[a] * zm[b];
    }
    double lam[3], v[3], lmid;
    d_eig3(cov, lam, v, &lmid);
    if (lam[2] > P.line_ratio * lam[1]) {
      double pa[3], pb[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) { pa[a] = P.line_half_len * v[a] + center[a]; pb[a] = -P.line_half_len * v[a] + center[a]; }
      lmb_put_edge(blk, pa, pb);
    }
  } else {  // :424-460
    double A[3][5], b[5], nrm[3];
    float mx[5], my[5], mz[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const float4 m = mp[bi[j]];
      mx[j] = m.x; my[j] = m.y; mz[j] = m.z;
      A[0][j] = m.x; A[1][j] = m.y; A[2][j] = m.z; b[j] = -1.0;
    }
    d_colpiv_qr53(A, b, nrm);   // :435
    const double nn = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    const double dd = 1 / nn;
#pragma unroll
    for (int a = 0; a < 3; ++a) nrm[a] /= nn;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (fabs(nrm[0] * mx[j] + nrm[1] * my[j] + nrm[2] * mz[j] + dd) > P.plane_tol) ok = false;
    if (ok) lmb_put_plane(blk, nrm, dd);
  }
  } while (false);
  }
}

// ---- the accepted residual rows of one registration --------------------------------------------------------------------------
// Round 3: lm_solve used to pack its ~2.9 k accepted rows (80 B each = 230 KB per stream) into HBM and stream them through every one
// of the ~30 evaluations of a mapping frame: 512 streams x 230 KB x 30 = 3.5 GB per launch out of the L2 / Infinity Cache, which is what
// bounded the kernel (514 us per launch with the rows, 0.94 MB of HBM traffic per scan).  Now the rows live in LDS for the whole solve,
// structure of arrays, edges apart from planes (lm_rows.h: the layouts, 60 B and 44 B a row): 143 KB at 16 x 1800.  Rows beyond the
// workgroup's LDS budget stay in `crows` as streamed records and are read
// from there — same arithmetic, same order.  The compaction is STABLE in the query index (every thread takes a contiguous range of
// queries), thread t evaluates edges t, t + T, ... and then planes t, t + T, ...: the summation order of the normal equations is a
// function of the accepted-query lists alone, and lm_shard_eval (all rows in `crows`) follows the same order.
// Measured on the 2048-stream bench (four stream groups share the chip), T threads x LDS for the rows, always against the other variants in
// the same run (runs on different boxes differ by +-3 %).  While map_update still flooded the chip with empty 68 KB workgroups: 512 x 158 KB 348 k
// scans/s, 256 x 158 KB 347 k, 256 x 96 KB 355 k, 256 x 48 KB 357 k, 256 x 0 354 k, 1024 x any 287 k (128 VGPRs: spills); the old kernel 349 k.
// After that fix: 256 x 96 KB 408 k, 256 x 32 KB 410 k, 256 x 0 409 k, 256 x 158 KB 399 k; 512 x 96 KB against 256 x 96 KB: 396 k / 404 k.
// The row budget does not matter except for the variant that needs a CU's whole LDS (it has to wait for every other LDS user to leave);
// 256 threads x 254 VGPRs leave half a CU's register file to the other stream groups.  A single stream's solve takes 94 us with 512 threads,
// ~130 us with 256, 150 us before.  Two thirds of the rows on chip remove two thirds of the kernel's HBM traffic: 256 threads, 96 KB.
#ifndef LM_SOLVE_T
#define LM_SOLVE_T 256
#endif
#define LM_SOLVE_RED_BYTES ((size_t)28 * (LM_SOLVE_T / 8) * sizeof(double))
#define LM_SOLVE_DYN_BYTES ((size_t)158 * 1024)   // upper limit (ALEGO_LM_ROW_LDS): of the CU's 160 KB; the kernel's static LDS (solver state, scan tables) is < 2 KB
#define LM_SOLVE_ROW_BYTES_DEFAULT ((size_t)96 * 1024)
template <int T>
DEV_INLINE void lm_pack_rows(const LmCtx& L, int slot, int nqc, int nqs, unsigned char* row_lds, size_t row_budget, int (*s_cnt)[T / 64], LmRows& W) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* blocks = lm_blocks_of(L, slot);
  const float4* qc = L.cur_corner_ds + (size_t)slot * L.kf_cap_c;
  const float4* qs = L.cur_total_ds + (size_t)slot * L.total_cap;
  const int n_all = nqc + nqs, per = (n_all + T - 1) / T;
  const int lo = min(tid * per, n_all), hi = min(lo + per, n_all);
  auto block_of = [&](int i) { return blocks + lm_row_of_query(i, nqc, L.kf_cap_c) * LMB_W; };
  constexpr int U = 4;   // loads in flight per thread
  int cc = 0, cs = 0;
  for (int i0 = lo; i0 < hi; i0 += U) {
    double ty[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ty[u] = block_of(min(i0 + u, n_all - 1))[LMB_TYPE];
#pragma unroll
    for (int u = 0; u < U; ++u) if (i0 + u < hi && ty[u] != 0.0) { if (i0 + u < nqc) ++cc; else ++cs; }
  }
  const int ic = wave_incl_scan(cc), is = wave_incl_scan(cs);
  if (lane == 63) { s_cnt[0][wave] = ic; s_cnt[1][wave] = is; }
  __syncthreads();
  int epos = ic - cc, ppos = is - cs, Rc = 0, Rs = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) { const int a = s_cnt[0][w], b = s_cnt[1][w]; if (w < wave) { epos += a; ppos += b; } Rc += a; Rs += b; }
  W = lml_make(Rc, Rs, row_lds, row_budget, lm_crows_of(L, slot));
  for (int i0 = lo; i0 < hi; i0 += U) {
    LmBlock B[U];
    float4 pt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = min(i0 + u, n_all - 1);
      B[u] = lmb_load(block_of(i));
      pt[u] = i < nqc ? qc[i] : qs[i - nqc];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u;
      if (i < hi && lmb_type(B[u]) != 0.0) {
        const bool is_c = i < nqc;
        const int r = is_c ? epos++ : ppos++;
        if (is_c && r < W.Ce) lml_put_edge(W, r, B[u], pt[u]);
        else if (!is_c && r < W.Cp) lml_put_plane(W, r, B[u], pt[u]);
        else lms_put(W.crows + (is_c ? lms_edge_at(r) : lms_plane_at(Rc, r)) * LMS_W, B[u], pt[u]);
      }
    }
  }
  __threadfence_block();
  __syncthreads();
}

// residuals + Jacobians of all rows at the pose of Tm, accumulated into this thread's 28 normal-equation scalars
// (FULL = false: the residuals alone, into acc[27] — the cost of a candidate point; same rows, same order)
// The two evaluations are lm_eval_edge / lm_eval_plane (lm_rows.h) written out: called from here, the same code behind a helper takes lm_solve
// from 254 to 255 VGPRs and lm_shard_eval from 2 to 3 wavefronts per SIMD (profiles/r13_solver_rows.md).
template <int T, bool FULL = true>
DEV_INLINE void lm_eval_rows(const LmRows& W, const PoseTerms& Tm, double huber, double acc[28]) {
  const double c3[3] = {0, 0, 0};
  for (int i = threadIdx.x; i < W.Rc; i += T) {
    LmEdge e;
    if (i < W.Ce) e = lml_edge(W, i); else e = lms_edge(W.crows + lms_edge_at(i) * LMS_W);
    if constexpr (FULL) {
      double res, J[6];
      eval_block(BLK_EDGE, e.p, e.a, e.b, c3, 0.0, Tm, &res, J);
      accumulate_block(res, J, huber, acc);
    } else accumulate_cost(eval_block_residual<BLK_EDGE>(e.p, e.a, e.b, c3, 0.0, Tm), huber, acc[27]);
  }
  for (int j = threadIdx.x; j < W.Rs; j += T) {
    LmPlane p;
    if (j < W.Cp) p = lml_plane(W, j); else p = lms_plane(W.crows + lms_plane_at(W.Rc, j) * LMS_W);
    if constexpr (FULL) {
      double res, J[6];
      eval_block(BLK_PLANE, p.p, p.n, c3, c3, p.d, Tm, &res, J);
      accumulate_block(res, J, huber, acc);
    } else accumulate_cost(eval_block_residual<BLK_PLANE>(p.p, p.n, c3, c3, p.d, Tm), huber, acc[27]);
  }
}

// wave 0, all 64 lanes, lane 6 i + j owning entry (i, j) (lanes 36 .. 63 shadow lane 35): the cyclic Jacobi of reg_cov_math.h on the lane-owned entries
// of the symmetric A — a rotation fetches its partners with wave shuffles, every lane forms (c, s) from the same three entries — and the ordering:
// lam[6] the eigenvalues ascending, ties by index (every lane holds all six); returns entry (i, j) of the eigenvectors sorted likewise.  The one
// decomposition of lm_regcov (rc_tail) and lm_solve_remap (rm_tail); the operations and their order are rc_jacobi's and rc_sort's, entry by entry.
// shfl(v, lane): the value of `lane`.  ShflHip is __shfl; ShflDirect forms ds_bpermute's byte address here — __shfl adds (lane id & ~63) to the source,
// a term of the lane alone: inside lm_solve_remap the compiler hoists it, and every index built on it, out of the solver's loops (rm_tail).
struct ShflHip { DEV_INLINE double operator()(double v, int src) const { return __shfl(v, src); } };
struct ShflDirect {
  DEV_INLINE double operator()(double v, int src) const {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(unsigned long long)b), hi = __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
  }
};
template <class Shfl>
DEV_INLINE double rc_eigen_lanes(double A, int i, int j, double lam[6], const Shfl& shfl) {
  double V = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < RC_SWEEPS_MAX; ++sweep) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a + 1; b < 6; ++b) { const double x = shfl(A, a * 6 + b); off += x * x; }
#pragma unroll
    for (int a = 0; a < 6; ++a) { const double x = shfl(A, a * 7); dg += x * x; }
    if (!(off > RC_OFF_REL * dg)) break;
#pragma unroll
    for (int pp = 0; pp < 5; ++pp)
#pragma unroll
      for (int q = pp + 1; q < 6; ++q) {
        const double apq = shfl(A, pp * 6 + q);
        if (apq == 0.0) continue;   // (uniform)
        double c, s;
        rc_rot_cs(shfl(A, pp * 7), shfl(A, q * 7), apq, &c, &s);
        { const double xp = shfl(A, i * 6 + pp), xq = shfl(A, i * 6 + q); A = rc_rot_col(j, pp, q, c, s, xp, xq, A); }
        { const double xp = shfl(A, pp * 6 + j), xq = shfl(A, q * 6 + j); A = rc_rot_row(i, pp, q, c, s, xp, xq, A); }
        { const double xp = shfl(V, i * 6 + pp), xq = shfl(V, i * 6 + q); V = rc_rot_col(j, pp, q, c, s, xp, xq, V); }
      }
  }
  // ascending order, ties by index: sorted column r is the column whose diagonal entry has rank r
  double dd[6];
  int rk[6], src = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) dd[k] = shfl(A, k * 7);
#pragma unroll
  for (int k = 0; k < 6; ++k) { rk[k] = rc_rank(dd, k); if (rk[k] == j) src = k; }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) v = rk[k] == r ? dd[k] : v;
    lam[r] = v;
  }
  return shfl(V, i * 6 + src);
}

// The spectrum of a registration on wave 0 (rc_spectrum of reg_cov_math.h, entry by entry; lane, l, i, j as above): the one front of rc_tail and rm_tail and the
// owner of their guards.  t6: rc_trig's six values at p (pose_terms_coop's table of the evaluation at p holds them, by the very calls rc_trig makes).  Returns the
// status; with 1, s_N holds N = M(p)^-1 and info, vs, lam[6], vi[6], vj[6] are this lane's entry of N^T H N, its entry of the sorted eigenvectors, the eigenvalues
// ascending and rows i and j of the sorted eigenvectors.  (lm_solve_remap sits at its 256 VGPRs: the caller passes the lane index through an opaque move, N goes to
// LDS through a select — 36 doubles in registers at a time — fenced by sched_barriers from what follows, and the shuffle is a template parameter: ShflDirect there.)
template <class Shfl>
DEV_INLINE int rc_front_lanes(const double* s_out /* LDS [28] */, const double* t6, const double* p, int n_edge, int n_plane, double* s_N /* LDS [36] */, int lane, int i, int j,
                              const Shfl& shfl, double* info, double* vs, double lam[6], double vi[6], double vj[6]) {
  if (n_edge + n_plane <= 6) return 0;
  if (fabs(t6[3]) < RC_COS_PITCH_MIN) return -3;
  {   // N = M^-1 into LDS (an entry of info indexes it by lane; a private array indexed that way would live in scratch)
    double N[36];
    rc_minv_t(t6, N);
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 36; ++k) v = lane == k ? N[k] : v;
    if (lane < 36) s_N[lane] = v;
    __threadfence_block();
  }
  __builtin_amdgcn_sched_barrier(0);
  *info = rc_info_entry(s_out, s_N, i < j ? i : j, i < j ? j : i);
  const bool bad = !rc_finite(*info) || (lane < 28 && !rc_finite(s_out[lane])) || (lane < 6 && !rc_finite(p[lane]));
  if (__any(bad)) return -2;
  __builtin_amdgcn_sched_barrier(0);
  *vs = rc_eigen_lanes(*info, i, j, lam, shfl);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 6; ++k) { vi[k] = shfl(*vs, i * 6 + k); vj[k] = shfl(*vs, j * 6 + k); }
  return 1;
}
// wave 0: a record without a result — its `count` doubles from `dv` zero but for the first `keep` of `head` (null: none); header(): lane 0 writes the ints
template <class Header> DEV_INLINE void rec_store_empty(double* dv, int count, const double* head, int keep, int lane, Header&& header) {
  for (int k = lane; k < count; k += 64) dv[k] = k < keep ? head[k] : 0.0;
  if (lane == 0) header();
}

// ---- solution remapping (alego_remap_enable; remap_math.h) ------------------------------------------------------------
// The projector of a mapping frame from the 28 sums of the solver's own first evaluation, on wave 0 between that evaluation and the control
// thread's first turn; it stays in LDS for every iteration of every outer solve of the frame.
// (What the tail needs of the frame lies in LDS next to it, written by thread 0 before the solve: carried in registers through the evaluations, where
// the kernel's register need peaks, it costs lm_solve_remap a wavefront per SIMD.)
struct RmLds {
  double P[36], N[36], M[36];   // P: what lm_step reads when `on` (something is held)
  double eig_min;
  alego_remap* rec;
  int on, first, n_edge, n_plane, frame;   // first: the frame's first evaluation has not been taken in yet
};
static_assert(offsetof(alego_remap, start) == 16 && sizeof(alego_remap) == 16 + 84 * sizeof(double), "rm_empty hands rec_store_empty the record's doubles from `start`");
template <bool REMAP> DEV_INLINE RmLds* rm_lds() {
  if constexpr (REMAP) { __shared__ RmLds R; return &R; }
  else return nullptr;
}
// the record's ints (lane 0), and wave 0's record without a result: nothing is held, `start` is kept
DEV_INLINE void rm_header(alego_remap* rec, int status, int n_held, int frame) { rec->status = status; rec->n_held = n_held; rec->frame = frame; rec->pad = 0; }
DEV_INLINE void rm_empty(alego_remap* rec, int status, int frame, const double* x0, int lane) { rec_store_empty(rec->start, 84, x0, 6, lane, [&] { rm_header(rec, status, 0, frame); }); }
// wave 0, all 64 lanes active, lane 6 i + j owning entry (i, j): the projector tail of rc_front_lanes.  The operations and their order are rm_compute's,
// entry by entry.  s_trig: pose_terms_coop's table of the evaluation at x0 — entries 6 .. 11 are cos, sin of roll, pitch, yaw by the very calls rc_trig makes.
DEV_INLINE void rm_tail(const double* s_out /* LDS [28] */, const double* s_trig /* LDS [12] */, RmLds& R, const double* x0, int n_edge, int n_plane, int frame, double eig_min, alego_remap* rec) {
  // (the lane index through an opaque move: everything below that depends on the lane alone — shuffle indices, entry selects — is invariant in the
  // solver's loops, and hoisted out of them it stays in ~50 registers through the evaluations, which costs the kernel a wavefront per SIMD)
  int lane = threadIdx.x;
  asm volatile("" : "+v"(lane));
  const int l = lane < 36 ? lane : 35, i = l / 6, j = l - 6 * i;
  const double t6[6] = {s_trig[7], s_trig[6], s_trig[9], s_trig[8], s_trig[11], s_trig[10]};   // rc_trig's order
  if (lane == 0) { R.on = 0; R.first = 0; }   // (once per frame)
  double info, vs, lam[6], vi[6], vj[6], col[6];
  const ShflDirect shfl;
  const int st = rc_front_lanes(s_out, t6, x0, n_edge, n_plane, R.N, lane, i, j, shfl, &info, &vs, lam, vi, vj);
  if (st != 1) { rm_empty(rec, st, frame, x0, lane); return; }
  __builtin_amdgcn_sched_barrier(0);
  {   // M into LDS, as N went: entries of P index it by lane (after N, not with it: 36 doubles in registers at a time)
    double M[36];
    rc_m_t(t6, M);
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 36; ++k) v = lane == k ? M[k] : v;
    if (lane < 36) R.M[lane] = v;
    __threadfence_block();
  }
  __builtin_amdgcn_sched_barrier(0);
  const double pt = rm_pt_entry(vi, vj, lam, eig_min);
#pragma unroll
  for (int a = 0; a < 6; ++a) {   // (Pt M)(a, j) for the six a of this lane's column
    double row[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) row[b] = shfl(pt, a * 6 + b);
    col[a] = rm_ptm_entry(row, R.M, j);
    __builtin_amdgcn_sched_barrier(0);   // (one row of shuffles in flight: all 36 hoisted to the front cost the kernel a wavefront per SIMD)
  }
  int held = 0;
  double lam_j = 0.0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 6; ++k) { bad = bad || !rc_finite(lam[k]); held += rm_kept(lam[k], eig_min) ? 0 : 1; lam_j = j == k ? lam[k] : lam_j; }
  const double pe = rm_p_entry(R.N, i, col);
  const double P = held == 0 ? (i == j ? 1.0 : 0.0) : (held == 6 ? 0.0 : pe);
  bad = bad || !rc_finite(vs) || !rc_finite(P);
  if (__any(bad)) { rm_empty(rec, -2, frame, x0, lane); return; }
  if (lane < 36) {
    R.P[l] = P; rec->eigvec[l] = vs; rec->proj[l] = P;
    if (i == 0) rec->eigval[j] = lam_j;
  }
  if (lane < 6) rec->start[lane] = x0[lane];
  if (lane == 0) { rm_header(rec, 1, held, frame); R.on = held > 0 ? 1 : 0; }
  __threadfence_block();
}
// wg_solve's hook (dev_cost.h): the decomposition behind the first evaluation of the frame, the projector for every step after it
struct RmHook {
  static constexpr bool remap = true;
  RmLds* R;
  DEV_INLINE void after_begin(const double* x0, const double* s_trig, const double* s_out) const {
    if (threadIdx.x < 64 && R->first) rm_tail(s_out, s_trig, *R, x0, R->n_edge, R->n_plane, R->frame, R->eig_min, R->rec);
  }
  DEV_INLINE const double* proj() const { return R->on ? R->P : nullptr; }
};

enum { LM_T_PACK = 4, LM_T_LD0 = 43 };   // -DALEGO_TIMING: the phases of lm_solve (dev_cost.h WG_T_*, and the pack) in ld[43 .. 47]
// scan2MapOptimization's solver part, one workgroup per stream.
// The normal equations are evaluated only where a step is computed from them: at the point a ceres::Solve starts from and at an adopted point
// the solve goes on from.  A candidate is evaluated for its cost (a third of a full row's instructions and one scalar to reduce instead of 28)
// unless the step before it was successful (ALEGO_SOLVE_SPECULATE, solve_rows.h: it is then evaluated in full at once);
// one that is rejected, or that ends the solve (cost change, step size, the last permitted iteration) never gets its Jacobian, and a further outer
// iteration that starts where the last one ended with the normal equations in hand takes them from there.  Every evaluation is a function of
// (x, rows): the points visited, their costs and the steps between them are what evaluating everything in full gives, bit for bit
// (FULL_EVAL: exactly that, the cross-check kernel behind ALEGO_SOLVE_FULL_EVAL=1; tests/test_solver_eval_split.py).
// REMAP (lm_solve_remap, alego_remap_enable): the steps of the whole frame are projected off the directions the first evaluation does not observe
// (the section above); every `if constexpr (REMAP)` below is absent from lm_solve and lm_solve_full_eval.
template <bool FULL_EVAL, bool REMAP = false>
DEV_INLINE void lm_solve_body(const DevCtx& d, const LmCtx& L) {
  const int slot = blockIdx.x + d.slot0;
  int* li = lip(L, slot);
  if (!li[LI_RUN]) return;
  const alego_params& P = d.P;
  double* ld = ldp(L, slot);
  if (lm_reg_skipped(li, P)) {
    if (threadIdx.x == 0) lm_store_skipped(li);
    if constexpr (REMAP) { if (threadIdx.x < 64) rm_empty(L.rm_rec + slot, 0, li[LI_FRAME], ld + LD_PARAMS, threadIdx.x); }
    return;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_smem[];
  double* s_acc = reinterpret_cast<double*>(lm_smem);                // [28][LM_SOLVE_T / 8]
  __shared__ double s_out[28], s_trig[12];
  __shared__ LmState S;
  __shared__ int s_action, s_again, s_cnt[2][LM_SOLVE_T / 64];
  // ---- correspondence counts (:465) and the accepted rows, into LDS ----
  LmRows W;
  WgClock<false> ck;
  ck.begin();
  lm_pack_rows<LM_SOLVE_T>(L, slot, li[LI_NCUR_C], li[LI_NTOTAL_DS], lm_smem + LM_SOLVE_RED_BYTES, L.solve_row_bytes, s_cnt, W);
  ck.end(LM_T_PACK);
  if (threadIdx.x == 0) { li[LI_NCC] = W.Rc; li[LI_NSC] = W.Rs; li[LI_OPTIMIZED] = 1; }
  const int R = W.Rc + W.Rs;
  auto rows = [&](const PoseTerms& T, double* acc, auto full) { lm_eval_rows<LM_SOLVE_T, decltype(full)::value>(W, T, P.huber_delta, acc); };
  if constexpr (REMAP) {
    if (threadIdx.x == 0) {
      RmLds& Rm = *rm_lds<REMAP>();
      Rm.eig_min = L.rm_eig_min; Rm.rec = L.rm_rec + slot; Rm.n_edge = W.Rc; Rm.n_plane = W.Rs; Rm.frame = li[LI_FRAME]; Rm.on = 0; Rm.first = 1;
    }
    if (R == 0 && threadIdx.x < 64) rm_empty(L.rm_rec + slot, 0, li[LI_FRAME], ld + LD_PARAMS, threadIdx.x);   // (no solve: the record of fewer than 7 rows)
  }
  for (int outer = 0; outer < P.lm_outer_iters; ++outer) {  // :360 — identical correspondences both times
    if (R == 0) {
      if (threadIdx.x == 0) lm_store_outer_empty(li, ld, outer);
      continue;
    }
    // (s_again: thread 0's verdict at the end of the outer iteration before, behind that iteration's closing barrier)
    if constexpr (REMAP) {
      const RmHook hook{rm_lds<REMAP>()};
      wg_solve<LM_SOLVE_T, 3, FULL_EVAL>(S, &s_action, (!FULL_EVAL && outer > 0 && s_again) ? LM_EV_AGAIN : LM_EV_BEGIN, ld + LD_PARAMS, P.lm_max_iters, s_trig, s_acc, s_out, rows, ck, hook);
    } else
    wg_solve<LM_SOLVE_T, 3, FULL_EVAL>(S, &s_action, (!FULL_EVAL && outer > 0 && s_again) ? LM_EV_AGAIN : LM_EV_BEGIN, ld + LD_PARAMS, P.lm_max_iters, s_trig, s_acc, s_out, rows, ck);
    if (threadIdx.x == 0) {
#ifdef ALEGO_TIMING
      for (int k = 0; k <= LM_T_PACK; ++k) ld[LM_T_LD0 + k] = (double)ck.tm[k];   // (accumulated over both outer iterations)
#endif
      lm_store_outer(li, ld, outer, S);
      s_again = S.jac_valid;   // a point adopted in the last permitted iteration has no normal equations yet: the next outer iteration evaluates it
    }
    __syncthreads();
  }
}
// grid (slots).  The default kernel keeps the plain name the profiles and the bench look up.
__global__ void __launch_bounds__(LM_SOLVE_T) lm_solve(DevCtx d, LmCtx L) { lm_solve_body<false>(d, L); }
__global__ void __launch_bounds__(LM_SOLVE_T) lm_solve_full_eval(DevCtx d, LmCtx L) { lm_solve_body<true>(d, L); }
// (two wavefronts per SIMD asked for: left to itself the compiler takes 256 VGPRs + 2 AGPRs and halves the occupancy; with the bound it fits 256 without scratch)
__global__ void __launch_bounds__(LM_SOLVE_T, 2) lm_solve_remap(DevCtx d, LmCtx L) { lm_solve_body<false, true>(d, L); }
__global__ void __launch_bounds__(LM_SOLVE_T, 2) lm_solve_remap_full_eval(DevCtx d, LmCtx L) { lm_solve_body<true, true>(d, L); }

// ---- covariance and degeneracy of the registration (alego_regcov_enable; reg_cov_math.h) -----------------------------
// One full evaluation of the accepted rows at the solver's final point, then the 6x6 part on wave 0.  The rows are streamed once from where
// lm_fit left them (L.blocks and the two query clouds), thread-strided over the QUERIES: thread t takes queries t, t + T, ... and the 28 sums
// go through block_reduce28, so the result is a function of the slot's rows alone.  (lm_solve packs the rows into LDS because it reads them
// ~30 times; one pass gains nothing from it.)
struct RcSrc {
  const double* blocks;      // block records (lm_rows.h)
  const float4 *qc, *qs;     // corner queries, surf queries
  int nqc, nqs, surf_row0;   // query i of the nqc + nqs: row lm_row_of_query(i, nqc, surf_row0)
  const double* params;      // p[6]
};
static_assert(offsetof(alego_regcov, cost) == 24 && sizeof(alego_regcov) == 24 + 122 * sizeof(double), "rc_empty hands rec_store_empty the record's doubles from `cost`");

// the record's ints (lane 0), and wave 0's record without a result
DEV_INLINE void rc_header(alego_regcov* rec, int status, int n_edge, int n_plane, int n_degenerate, int frame) {
  rec->status = status; rec->n_edge = n_edge; rec->n_plane = n_plane; rec->n_degenerate = n_degenerate; rec->frame = frame; rec->pad = 0;
}
DEV_INLINE void rc_empty(alego_regcov* rec, int st, int n_edge, int n_plane, int frame) { rec_store_empty(&rec->cost, 122, nullptr, 0, threadIdx.x, [&] { rc_header(rec, st, n_edge, n_plane, 0, frame); }); }

// wave 0, all 64 lanes active.  Lane 6 i + j owns entry (i, j) of info, of the eigenvectors and of cov (lanes 36 .. 63 shadow lane 35 and store
// nothing): the covariance tail of rc_front_lanes.  The operations and their order are rc_compute's (reg_cov_math.h), entry by entry.
// s_trig: pose_terms_coop's table of the evaluation at p, as for rm_tail.
DEV_INLINE void rc_tail(const double* s_out /* LDS [28] */, const double* s_trig, double* s_N /* LDS [36] */, const double* p, int n_edge, int n_plane, int frame, const double* opt, alego_regcov* rec) {
  const int lane = threadIdx.x, l = lane < 36 ? lane : 35, i = l / 6, j = l - 6 * i;
  const double t6[6] = {s_trig[7], s_trig[6], s_trig[9], s_trig[8], s_trig[11], s_trig[10]};   // rc_trig's order
  double info, vs, lam[6], w[6], vi[6], vj[6];
  const int st = rc_front_lanes(s_out, t6, p, n_edge, n_plane, s_N, lane, i, j, ShflHip{}, &info, &vs, lam, vi, vj);
  if (st != 1) { rc_empty(rec, st, n_edge, n_plane, frame); return; }
  const double s2 = rc_sigma2(s_out[27], n_edge + n_plane, opt[RC_SIGMA0]);
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = rc_weight(lam[k], lam[5], opt[RC_LAMBDA_FLOOR]);
  const double cv = s2 * rc_cov_entry(vi, vj, w);
  bool bad = !rc_finite(s2) || !rc_finite(vs) || !rc_finite(cv);
  int ndeg = 0;
  double lam_j = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) { bad = bad || !rc_finite(lam[k]); ndeg += lam[k] < opt[RC_EIG_MIN] ? 1 : 0; lam_j = j == k ? lam[k] : lam_j; }
  if (__any(bad)) { rc_empty(rec, -2, n_edge, n_plane, frame); return; }
  if (lane < 36) {
    rec->info[l] = info; rec->eigvec[l] = vs; rec->cov[l] = cv;
    if (i == 0) rec->eigval[j] = lam_j;
    if (i == j) rec->variance[i] = rc_clamp(opt[RC_SCALE] * cv, opt[RC_VAR_MIN + i], opt[RC_VAR_MAX + i]);
  }
  if (lane == 0) { rc_header(rec, 1, n_edge, n_plane, ndeg, frame); rec->cost = s_out[27]; rec->sigma2 = s2; }
}

template <int T>
DEV_INLINE void rc_body(const RcSrc& S, double huber, const double* opt, int frame, alego_regcov* rec) {
  __shared__ double s_acc[28 * (T / 8)], s_out[28], s_trig[12], s_N[36];
  __shared__ int s_n[2];
  const int tid = threadIdx.x;
  if (tid < 2) s_n[tid] = 0;   // (published by the barrier of the pose terms)
  auto rows = [&](const PoseTerms& Tm, double* acc, auto) {
    const int n_all = S.nqc + S.nqs;
    int ne = 0, np = 0;
    for (int q = tid; q < n_all; q += T) {
      const LmBlock B = lmb_load(S.blocks + lm_row_of_query(q, S.nqc, S.surf_row0) * LMB_W);
      if (lmb_type(B) == 0.0) continue;
      if (q < S.nqc) { lm_eval_edge<true>(lm_edge_of(B, S.qc[q]), Tm, huber, acc); ++ne; }
      else { lm_eval_plane<true>(lm_plane_of(B, S.qs[q - S.nqc]), Tm, huber, acc); ++np; }
    }
    if (ne) atomicAdd(&s_n[0], ne);
    if (np) atomicAdd(&s_n[1], np);
  };
  WgClock<false> ck;
  wg_evaluate<T, 3, true>(S.params, s_trig, s_acc, s_out, rows, ck);   // (ends with a barrier: the counts are complete)
  if (tid >= 64) return;
  rc_tail(s_out, s_trig, s_N, S.params, s_n[0], s_n[1], frame, opt, rec);
}

// grid (slots), between the solver and lm_finish (which overwrites LD_PARAMS with the f32 key pose when it saves a frame).  A slot without a mapping
// frame keeps its record (its `frame` tells); one the solver skipped (LI_FLAGS & 16) gets status 0.
__global__ void __launch_bounds__(LM_SOLVE_T) lm_regcov(DevCtx d, LmCtx L) {
  const int slot = blockIdx.x + d.slot0;
  const int* li = lip(L, slot);
  if (!li[LI_RUN]) return;
  alego_regcov* rec = L.rc_rec + slot;
  if (!li[LI_OPTIMIZED]) { if (threadIdx.x < 64) rc_empty(rec, 0, 0, 0, li[LI_FRAME]); return; }
  const RcSrc S{lm_blocks_of(L, slot), L.cur_corner_ds + (size_t)slot * L.kf_cap_c, L.cur_total_ds + (size_t)slot * L.total_cap,
                li[LI_NCUR_C], li[LI_NTOTAL_DS], L.kf_cap_c, ldp(L, slot) + LD_PARAMS};
  rc_body<LM_SOLVE_T>(S, d.P.huber_delta, L.rc_opt, li[LI_FRAME], rec);
}
// the same on caller-supplied rows (alego_debug_regcov)
__global__ void __launch_bounds__(LM_SOLVE_T) lm_regcov_debug(RcSrc S, double huber, const double* opt, alego_regcov* rec) { rc_body<LM_SOLVE_T>(S, huber, opt, 0, rec); }

// grid (ceil(slots/64)): saveKeyFramesAndFactor :491-559 (no-loop-closure pass-through) + transformUpdate :481-489
__global__ void lm_finish(DevCtx d, LmCtx L) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_launch) return;
  const int slot = s + d.slot0;
  int* li = lip(L, slot);
  if (!li[LI_RUN]) return;
  li[LI_REBUILD] = 0;   // the map sequence of this frame is done: no stale flag for a later round over the group's jobs
  double* ld = ldp(L, slot);
  const int nkf = li[LI_NKF];
  bool add = !L.loc_on;   // localisation never saves a key frame: the optimised params_ reach transformUpdate as they are
  if (L.loc_on && li[LI_REC_CNT] == 0) return;   // ... and off the map (empty window) map -> odom stays what it was: dead reckoning
  if (nkf > 0) {
    const float* pre = kf_pose_of(L, kf_row(L, slot, nkf - 1));
    const double ex = ld[LD_T_M2L + 0] - (double)pre[0], ey = ld[LD_T_M2L + 1] - (double)pre[1], ez = ld[LD_T_M2L + 2] - (double)pre[2];
    if (ex * ex + ey * ey + ez * ez < d.P.min_keyframe_dist) add = false;  // :501-508
  }
  if (add) {
    double R[9];
    dq_to_mat(ldq(ld + LD_Q_M2L), R);
    const double roll = atan2(R[7], R[8]);
    const double pitch = atan2(-R[6], sqrt(R[7] * R[7] + R[8] * R[8]));
    const double yaw = atan2(R[3], R[0]);
    float* kp = kf_pose_of(L, kf_row(L, slot, nkf));
    kp[0] = (float)ld[LD_T_M2L + 0]; kp[1] = (float)ld[LD_T_M2L + 1]; kp[2] = (float)ld[LD_T_M2L + 2];
    kp[3] = (float)roll; kp[4] = (float)pitch; kp[5] = (float)yaw;
    for (int k = 0; k < 6; ++k) ld[LD_PARAMS + k] = (double)kp[k];  // :539-544
    li[LI_NKF] = nkf + 1; li[LI_DIRTY] = 1; li[LI_KF_ADDED] = 1; li[LI_FLAGS] |= 32;
  }
  // transformUpdate
  const DQuat qm2l = dq_zyx(ld[LD_PARAMS + 5], ld[LD_PARAMS + 4], ld[LD_PARAMS + 3]);
  stq(ld + LD_Q_M2L, qm2l);
  for (int k = 0; k < 3; ++k) ld[LD_T_M2L + k] = ld[LD_PARAMS + k];
  const DQuat qm2o = dq_mul(qm2l, dq_inverse(ldq(ld + LD_Q_O2L)));
  stq(ld + LD_Q_M2O, qm2o);
  double r[3];
  dq_rotate(qm2o, ld + LD_T_O2L, r);
  for (int k = 0; k < 3; ++k) ld[LD_T_M2O + k] = ld[LD_T_M2L + k] - r[k];
}

// grid (8, 3, slots): a key frame enters the ring (saveKeyFramesAndFactor :546-555 keeps the down-sampled clouds of the
// frame in the sensor frame; extractSurroundingKeyFrames :216-218,:240-242 transforms them by the f32 key pose,
// laserMapping.h:164-177).  The raw clouds go to ring entry f % KR (what the host pose graph reads back and what a corrected
// key pose is applied to); the transformed clouds go to kf_tmp_* (corner | surf followed by outlier) and are sorted by voxel key
// into the ring by the next VoxelGrid round (LI_KF_PENDING).
//   only_ring < 0: the slots whose LI_KF_ADDED is set store their current scan
//   only_ring >= 0: re-transform ring entry `only_ring` of every slot of the launch from its raw clouds (set_keypose / add_keyframe)
__global__ void __launch_bounds__(LM_BLOCK) lm_store_kf(DevCtx d, LmCtx L, int only_ring) {
  const int slot = blockIdx.z + d.slot0, kind = blockIdx.y;
  int* li = lip(L, slot);
  if (only_ring < 0 && !li[LI_KF_ADDED]) return;
  kf_row_to_tmp<LM_BLOCK>(L, slot, only_ring < 0 ? kf_entry(L, li[LI_NKF] - 1) : only_ring, kind, only_ring < 0);
}

// one thread: correctPoses :579-580 on map -> odom with the 3x4 [R | c] of the loop-closure correction
__global__ void lm_apply_correction(DevCtx d, LmCtx L, int slot, const double* rc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double* ld = ldp(L, slot);
  dq_apply_correction(ld + LD_Q_M2O, ld + LD_T_M2O, rc);
}


// ---------------------------------------------------------------------------------------------------------------------
// One registration sharded over the ranks of a communicator (BASELINE config 5): lm_knn / lm_fit above only fill the
// rows of this rank's query slice; the solver of lm_solve is cut at its evaluations so that the 28 normal-equation scalars (and,
// with the first evaluation, the two correspondence counts) can be summed over the ranks between the kernels:
//   lm_shard_pack            registration guard, packed rows of this rank, row counts
//   lm_shard_eval(which)     residual + Jacobian rows of this rank at params_ (which = 0) or at the candidate of the step in flight
//                            (which = 1) -> shard_part[slot][0..27] (+ counts in [28], [29])
//   ncclAllReduce(f64, sum)  over shard_part of all slots of the launch, on the same stream (host, lm_host.hip)
//   lm_shard_step(first)     the trust-region control of lm_solve on the summed scalars: identical on every rank, so all ranks
//                            take the same step; state (LmState) lives in HBM between the kernels
// The host enqueues the worst-case sequence (lm_outer_iters x (1 + lm_max_iters) evaluations); kernels of a finished solve return at once.
// Same evaluation code, same row order and same reduction as lm_solve: with one rank the result is bit-identical to it.
static_assert(sizeof(LmState) <= 64 * sizeof(double), "LmHost allocates 64 doubles per slot for the sharded solve's state");
DEV_INLINE void lm_shard_pack_dev(const DevCtx& d, const LmCtx& L, int slot) {
  int* li = lip(L, slot);
  int* ctl = L.shard_ctl + (size_t)slot * 8;
  double* part = L.shard_part + (size_t)slot * 32;
  if (threadIdx.x < 32) part[threadIdx.x] = 0.0;
  if (threadIdx.x == 0) { ctl[0] = 0; ctl[1] = LM_STOP; ctl[2] = 1; ctl[3] = 0; ctl[4] = 1; ctl[5] = 0; }
  if (!li[LI_RUN]) return;
  const alego_params& P = d.P;
  if (lm_reg_skipped(li, P)) {
    if (threadIdx.x == 0) lm_store_skipped(li);
    return;
  }
  __shared__ int s_cnt[2][LM_SOLVE_T / 64];
  LmRows W;
  lm_pack_rows<LM_SOLVE_T>(L, slot, li[LI_NCUR_C], li[LI_NTOTAL_DS], nullptr, 0, s_cnt, W);   // every row to HBM, in lm_solve's order
  if (threadIdx.x == 0) {
    ctl[0] = W.Rc + W.Rs; ctl[5] = W.Rc; ctl[1] = LM_EVAL; ctl[2] = 0; ctl[4] = 0;
    part[28] = (double)W.Rc; part[29] = (double)W.Rs;   // summed over the ranks with the first evaluation
    li[LI_OPTIMIZED] = 1;
  }
}
__global__ void __launch_bounds__(LM_SOLVE_T) lm_shard_pack(DevCtx d, LmCtx L) { lm_shard_pack_dev(d, L, blockIdx.x + d.slot0); }

DEV_INLINE void lm_shard_step_dev(const DevCtx& d, const LmCtx& L, int slot, int first);
DEV_INLINE void lm_shard_next_outer_dev(const LmCtx& L, int slot);
// pre (round 6: what used to be separate one-thread-per-slot launches between two evaluations runs at the head of the next evaluation's own workgroup, so an
// evaluation is ONE launch around its all-reduce instead of two or three):  LM_PRE_PACK = lm_shard_pack (the first evaluation of a frame), LM_PRE_STEP_FIRST /
// LM_PRE_STEP = lm_shard_step on the sums the all-reduce has just delivered, LM_PRE_STEP_NEXT = that step followed by lm_shard_next_outer (the first evaluation of
// a further outer iteration); LM_PRE_STEP_FIRST_NEXT = the same when the sums are those of the evaluation at params_ (lm_max_iters = 0: the inner loop was empty, so
// the step that closes the outer iteration is its first one, lm_begin included, as in lm_solve).  A workgroup is one slot: its thread 0 does exactly what the slot's thread of the separate launch did.
enum { LM_PRE_NONE = 0, LM_PRE_PACK, LM_PRE_STEP_FIRST, LM_PRE_STEP, LM_PRE_STEP_NEXT, LM_PRE_STEP_FIRST_NEXT };
__global__ void __launch_bounds__(LM_SOLVE_T) lm_shard_eval(DevCtx d, LmCtx L, int which, int pre) {
  const int slot = blockIdx.x + d.slot0;
  if (pre == LM_PRE_PACK) lm_shard_pack_dev(d, L, slot);
  else if (pre != LM_PRE_NONE && threadIdx.x == 0) {
    lm_shard_step_dev(d, L, slot, (pre == LM_PRE_STEP_FIRST || pre == LM_PRE_STEP_FIRST_NEXT) ? 1 : 0);
    if (pre == LM_PRE_STEP_NEXT || pre == LM_PRE_STEP_FIRST_NEXT) lm_shard_next_outer_dev(L, slot);
  }
  if (pre != LM_PRE_NONE) { __threadfence_block(); __syncthreads(); }   // (the control words, the candidate and the packed rows are read back by the whole workgroup)
  const int* ctl = L.shard_ctl + (size_t)slot * 8;
  if (ctl[2] || ctl[4] || ctl[1] != LM_EVAL) return;   // solve finished / guard failed: the all-reduce still runs, on stale partials nobody reads
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_smem[];
  double* s_acc = reinterpret_cast<double*>(lm_smem);
  __shared__ double s_out[28], s_trig[12];
  const LmState* S = reinterpret_cast<const LmState*>(L.shard_state) + slot;
  const double* ld = ldp(L, slot);
  double x[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = which == 0 ? ld[LD_PARAMS + k] : S->cand[k];
  const LmRows W = lml_make(ctl[5], ctl[0] - ctl[5], nullptr, 0, lm_crows_of(L, slot));   // (nothing resident)
  auto rows = [&](const PoseTerms& T, double* acc, auto) { lm_eval_rows<LM_SOLVE_T>(W, T, d.P.huber_delta, acc); };
  WgClock<false> ck;
  wg_evaluate<LM_SOLVE_T, 3, true>(x, s_trig, s_acc, s_out, rows, ck);
  double* part = L.shard_part + (size_t)slot * 32;
  if (threadIdx.x < 28) part[threadIdx.x] = s_out[threadIdx.x];
  if (threadIdx.x == 0 && which == 1) { part[28] = 0.0; part[29] = 0.0; }
}

// one thread per slot.  first: the evaluation just summed was the one at params_ (start of an outer iteration)
DEV_INLINE void lm_shard_step_dev(const DevCtx& d, const LmCtx& L, int slot, int first) {
  int* ctl = L.shard_ctl + (size_t)slot * 8;
  if (ctl[4]) return;
  int* li = lip(L, slot);
  double* ld = ldp(L, slot);
  LmState& S = reinterpret_cast<LmState*>(L.shard_state)[slot];
  const double* red = L.shard_part + (size_t)slot * 32;   // summed over the ranks
  const int outer = ctl[3];
  if (first) {
    if (outer == 0) { li[LI_NCC] = (int)(red[28] + 0.5); li[LI_NSC] = (int)(red[29] + 0.5); }
    if (li[LI_NCC] + li[LI_NSC] == 0) {
      lm_store_outer_empty(li, ld, outer);
      ctl[2] = 1; ctl[1] = LM_STOP;
      return;
    }
    double x0[6];
    for (int k = 0; k < 6; ++k) x0[k] = ld[LD_PARAMS + k];
    lm_begin(S, x0, red, d.P.lm_max_iters);
    ctl[2] = 0;
  } else {
    if (ctl[2] || ctl[1] != LM_EVAL) return;
    if (lm_consume(S, red) == LM_STOP) ctl[2] = 1;
  }
  int act = LM_STOP;
  if (!ctl[2]) { do { act = lm_propose(S); } while (act == LM_AGAIN); }
  ctl[1] = act;
  if (act == LM_STOP) {   // this outer iteration's ceres::Solve has returned
    ctl[2] = 1;
    lm_store_outer(li, ld, outer, S);
  }
}

__global__ void lm_shard_step(DevCtx d, LmCtx L, int first) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < d.n_launch) lm_shard_step_dev(d, L, s + d.slot0, first);
}
// between two outer iterations: the next ceres::Solve starts from the params_ the last one left (:360)
DEV_INLINE void lm_shard_next_outer_dev(const LmCtx& L, int slot) {
  int* ctl = L.shard_ctl + (size_t)slot * 8;
  if (ctl[4]) return;
  ctl[3] += 1; ctl[2] = 0; ctl[1] = LM_EVAL;
}

size_t lm_solve_row_bytes_max() { return LM_SOLVE_DYN_BYTES - LM_SOLVE_RED_BYTES; }
size_t lm_solve_row_bytes_default() { return LM_SOLVE_ROW_BYTES_DEFAULT; }
int lm_configure() {
  for (const void* k : {reinterpret_cast<const void*>(lm_solve), reinterpret_cast<const void*>(lm_solve_full_eval), reinterpret_cast<const void*>(lm_solve_remap),
                        reinterpret_cast<const void*>(lm_solve_remap_full_eval)})
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LM_SOLVE_DYN_BYTES) != hipSuccess) return -1;
  return 0;
}

// ---- launchers ---------------------------------------------------------------------
void launch_lm_prepare(const DevCtx& d, const LmCtx& L, int stage, int run_hint, int par, hipStream_t st) {
  // a frame that is not mapped only needs the odometry hand-over (one thread per slot); so does every frame whose clouds lm_stage copied
  const bool small = run_hint == 0 || stage == 2;
  const dim3 grid = small ? dim3(1, 1, d.n_launch) : dim3(8, 3, d.n_launch);
  ALEGO_LAUNCH(lm_prepare, grid, dim3(small ? 64 : LM_BLOCK), 0, st, d, L, stage, run_hint, par);
}
void launch_lm_stage(const DevCtx& d, const LmCtx& L, int run_hint, int par, hipStream_t st) {
  const dim3 grid = run_hint == 0 ? dim3(1, 1, d.n_launch) : dim3(8, 3, d.n_launch);
  ALEGO_LAUNCH(lm_stage, grid, dim3(run_hint == 0 ? 64 : LM_BLOCK), 0, st, d, L, run_hint, par);
}
void launch_lm_concat(const DevCtx& d, const LmCtx& L, hipStream_t st) {
  ALEGO_LAUNCH(lm_concat, dim3(2, L.K, d.n_launch), dim3(LM_BLOCK), 0, st, d, L);
}
void launch_lm_total(const DevCtx& d, const LmCtx& L, hipStream_t st) {
  ALEGO_LAUNCH(lm_total, dim3(8, d.n_launch), dim3(LM_BLOCK), 0, st, d, L);
}
void launch_lm_total_merge(const DevCtx& d, const LmCtx& L, const LtLists& W, hipStream_t st) {
  ALEGO_LAUNCH(lm_total_merge, dim3(d.n_launch), dim3(LT_T), 0, st, d, L, W);
}
void launch_lm_grid(const DevCtx& d, const LmCtx& L, hipStream_t st) {
  ALEGO_LAUNCH(lm_grid_build, dim3(2, d.n_launch), dim3(LM_BLOCK), 0, st, d, L);
}
// the solver kernel alone on the slots of d: lm_solve, its ALEGO_SOLVE_FULL_EVAL twin, or the _remap variant of either
void launch_lm_solve(const DevCtx& d, const LmCtx& L, bool remap, hipStream_t st) {
  const size_t lds = LM_SOLVE_RED_BYTES + L.solve_row_bytes;
  if (remap) {
    if (d.opt_solve_full_eval) ALEGO_LAUNCH(lm_solve_remap_full_eval, dim3(d.n_launch), dim3(LM_SOLVE_T), lds, st, d, L);
    else ALEGO_LAUNCH(lm_solve_remap, dim3(d.n_launch), dim3(LM_SOLVE_T), lds, st, d, L);
  } else if (d.opt_solve_full_eval) {
    ALEGO_LAUNCH(lm_solve_full_eval, dim3(d.n_launch), dim3(LM_SOLVE_T), lds, st, d, L);
  } else {
    ALEGO_LAUNCH(lm_solve, dim3(d.n_launch), dim3(LM_SOLVE_T), lds, st, d, L);
  }
}
// allreduce(buffer, count of doubles, stream): sums shard_part over the ranks in place (RCCL, lm_host.hip); nullptr = not sharded
// Returns the first non-zero allreduce code: a failed collective (communicator aborted, peer gone) would leave the ranks stepping on
// un-summed partials and hanging in the next one, so nothing further of this frame is enqueued and the caller reports the error.
int launch_lm_register(const DevCtx& d, const LmCtx& L, hipStream_t st, int (*allreduce)(void*, double*, size_t, hipStream_t), void* ar_ctx) {
  ALEGO_LAUNCH(lm_knn, dim3(lm_reg_grid(d, LM_ASSOC_GX)), dim3(128), 0, st, d, L);
  ALEGO_LAUNCH(lm_fit, dim3(lm_reg_grid(d, LM_FIT_GX)), dim3(128), 0, st, d, L);
  if (allreduce) {
    double* part = L.shard_part + (size_t)d.slot0 * 32;
    const size_t cnt = (size_t)d.n_launch * 32;
    const dim3 g1((d.n_launch + 63) / 64), b1(64);
    // per evaluation ONE launch + the all-reduce (round 6; before: pack | eval, all-reduce, step | next_outer as separate launches — 86 launches per mapping frame,
    // now 43): the step on the sums of evaluation k runs at the head of evaluation k + 1's workgroups, a last stand-alone step closes the frame
    const int pre_next = d.P.lm_max_iters <= 0 ? (int)LM_PRE_STEP_FIRST_NEXT : (int)LM_PRE_STEP_NEXT;   // (the evaluation before it: at params_ when the inner loop is empty)
    for (int outer = 0; outer < d.P.lm_outer_iters; ++outer) {
      ALEGO_LAUNCH(lm_shard_eval, dim3(d.n_launch), dim3(LM_SOLVE_T), LM_SOLVE_RED_BYTES, st, d, L, 0, outer == 0 ? (int)LM_PRE_PACK : pre_next);
      if (int rc = allreduce(ar_ctx, part, cnt, st)) return rc;
      for (int it = 0; it < d.P.lm_max_iters; ++it) {
        ALEGO_LAUNCH(lm_shard_eval, dim3(d.n_launch), dim3(LM_SOLVE_T), LM_SOLVE_RED_BYTES, st, d, L, 1, it == 0 ? (int)LM_PRE_STEP_FIRST : (int)LM_PRE_STEP);
        if (int rc = allreduce(ar_ctx, part, cnt, st)) return rc;
      }
    }
    ALEGO_LAUNCH(lm_shard_step, g1, b1, 0, st, d, L, d.P.lm_max_iters <= 0 ? 1 : 0);
  } else launch_lm_solve(d, L, L.rm_rec != nullptr, st);   // (alego_remap_enable picks the _remap variant; nothing of it is launched without it)
  if (L.rc_rec) ALEGO_LAUNCH(lm_regcov, dim3(d.n_launch), dim3(LM_SOLVE_T), 0, st, d, L);   // (alego_regcov_enable; nothing is launched without it)
  ALEGO_LAUNCH(lm_finish, dim3((d.n_launch + 63) / 64), dim3(64), 0, st, d, L);
  if (L.loc_on) return 0;  // no key frame is ever stored, sorted or archived
  ALEGO_LAUNCH(lm_store_kf, dim3(8, 3, d.n_launch), dim3(LM_BLOCK), 0, st, d, L, -1);
  if (L.arc_frames_cap > 0) launch_map_archive(d, L, 0, st);   // (alego_map_enable; nothing is launched without it)
  return 0;
}
// host twins (alego_regcov_host, alego_regcov_normal_host): rc_compute on the caller's 28 scalars; the functors of solve_rows.h over the caller's rows
void regcov_host(const double* acc28, const double* params6, int n_edge, int n_plane, const double* opt, alego_regcov* out) {
  std::memset(out, 0, sizeof(*out));
  out->n_edge = n_edge; out->n_plane = n_plane;
  out->status = rc_compute(acc28, params6, n_edge, n_plane, opt, &out->sigma2, out->info, out->eigval, out->eigvec, out->cov, out->variance, &out->n_degenerate, nullptr);
  if (out->status == 1) out->cost = acc28[27];
}
// alego_remap_host: rm_compute (remap_math.h) on the caller's 28 scalars
void remap_host(const double* acc28, const double* params6, int n_edge, int n_plane, double eig_min, alego_remap* out) {
  std::memset(out, 0, sizeof(*out));
  for (int k = 0; k < 6; ++k) out->start[k] = params6[k];
  out->status = rm_compute(acc28, params6, n_edge, n_plane, eig_min, out->eigval, out->eigvec, out->proj, &out->n_held);
}
// alego_remap_step_host: one lm_step (solve_rows.h) at x = 0 from given normal equations, scale and radius.  step6: the candidate, i.e. the step in
// parameter space (scale_i step_i, as lm_step forms it); returns lm_step's answer (LM_EVAL, or LM_AGAIN for an invalid step: step6 and mcc are then zero)
int remap_step_host(const double* H21, const double* g6, const double* scale6, double radius, const double* proj36, double* step6, double* mcc) {
  LmState S;
  std::memset(&S, 0, sizeof S);
  for (int k = 0; k < 21; ++k) S.H[k] = H21[k];
  for (int k = 0; k < 6; ++k) { S.g[k] = g6[k]; S.scale[k] = scale6[k]; }
  S.radius = radius; S.dec = 2.0;
  const int act = lm_step<true>(S, proj36);
  for (int k = 0; k < 6; ++k) step6[k] = act == LM_EVAL ? S.cand[k] : 0.0;
  *mcc = act == LM_EVAL ? S.mcc : 0.0;
  return act;
}
void regcov_normal_host(const double* params6, const double* edge_rows9, int n_edge, const double* plane_rows7, int n_plane, double huber, double* acc28) {
  for (int k = 0; k < 28; ++k) acc28[k] = 0.0;
  const PoseTerms Tm = pose_terms(params6);
  for (int i = 0; i < n_edge; ++i) {
    const double* r = edge_rows9 + (size_t)i * 9;
    lm_eval_edge<true>(LmEdge{{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}}, Tm, huber, acc28);
  }
  for (int i = 0; i < n_plane; ++i) {
    const double* r = plane_rows7 + (size_t)i * 7;
    lm_eval_plane<true>(LmPlane{{r[0], r[1], r[2]}, r[3], {r[4], r[5], r[6]}}, Tm, huber, acc28);
  }
}
void launch_lm_regcov_debug(const double* blocks, const float4* qc, int n_edge, const float4* qs, int n_plane, const double* params, double huber, const double* opt,
                            alego_regcov* rec, hipStream_t st) {
  const RcSrc S{blocks, qc, qs, n_edge, n_plane, n_edge, params};
  ALEGO_LAUNCH(lm_regcov_debug, dim3(1), dim3(LM_SOLVE_T), 0, st, S, huber, opt, rec);
}
void launch_lm_retransform(const DevCtx& d, const LmCtx& L, int ring, hipStream_t st) {
  ALEGO_LAUNCH(lm_store_kf, dim3(8, 3, d.n_launch), dim3(LM_BLOCK), 0, st, d, L, ring);
}
void launch_lm_apply_correction(const DevCtx& d, const LmCtx& L, int slot, const double* rc_dev, hipStream_t st) {
  ALEGO_LAUNCH(lm_apply_correction, dim3(1), dim3(64), 0, st, d, L, slot, rc_dev);
}
