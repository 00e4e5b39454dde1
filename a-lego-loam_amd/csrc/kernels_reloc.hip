// kernels_reloc.hip — alego_loc_relocalize: slots of a localising handle are placed in the frozen key-frame map
// without an initial pose.  The rule is reloc_math.h's; everything here returns exactly what its brute force returns.
//
//   rl_desc      one workgroup per map frame (at alego_reloc_enable), per listed slot, or per pending (slot, archived frame) of the
//                appearance search — a view of the frame's clouds each (KfClouds, kf_store.h): every point is read once, binned, and its
//                code raised into an LDS word per bin with atomicMax (a maximum of integers does not depend on the order); the tile is
//                then packed to bytes and the ring key summed from it
//   rl_bound     one thread per (query, frame): B = sum over rings of |keyQ - keyM| (<= dist(Q, M, s) for every s)
//   la_elig      (appearance search) one thread per (query, frame): B <- RL_INELIGIBLE unless the frame is eligible
//   rl_pick      one workgroup per query: the n_cand eligible frames smallest in (B, id)
//   rl_search    the hot path.  One wavefront per (query, frame) pair of a list, ONE LANE PER SHIFT: Q sits twice over in LDS (120 columns of
//                5 words), so lane s reads column c + s — 5 words apart from its neighbour, and 5 is coprime to the 64 banks: no conflicts —
//                while M's 300 words are wave-uniform (scalar loads).  v_sad_u8 sums four absolute byte differences per instruction; the
//                wave arg-min of (dist << 8 | s) gives D and the smallest s attaining it.
//   rl_list2     one workgroup per query: tau = the largest D among the n_cand frames rl_pick chose; the list of ALL frames with B <= tau, in id
//                order.  A frame with B > tau has D >= B > tau: it can neither enter the n_cand smallest (D, id) nor tie with them.
//   rl_topk      one workgroup per query: the n_cand smallest (D, id) of the second list, as candidate words (reloc_math.h)
//   rl_gather    verification: the slot's current scan under the guess (source) and the map frames around the candidate under their key poses
//                (raw sub-map), from the map store through kf_store.h's views; the rounds (loop_rounds), VoxelGrid, lc_grid and lc_icp are
//                kernels_loop.hip's (loop_ctx.h)
//   rl_apply     one lane per accepted slot: map -> odom corrected as lm_apply_correction does, params_ replaced
//   ma_mask      (alego_map_align) one thread per (query, frame): B <- RL_INELIGIBLE for every frame of a query whose ring key is all zero
//   ma_plan      (alego_map_align) one thread per (pair, query, candidate): the LcDet of the attempt from both archives' tables and the source key pose
//   ma_consensus (alego_map_align) one wavefront per pair, one lane per hypothesis: align_math.h's agreement, support, best and inliers with
//                wave.h's reductions; no LDS, no atomics
// Phase boundaries are kernel boundaries; no workgroup waits for another.
//
// Every query of the search kernels has a record (RlQuery): its row of the query descriptors, the first row and the number of the map
// rows it is searched in, and where its rows of the scratch start.  Relocalisation searches every query in rows 0 .. N - 1 of one map.
//
// alego_loop_search_appearance is the same search for the slots of a SLAM handle against their OWN archive, for
// revisits that detectLoopClosure's radius (kernels_loop.hip) cannot find because the drift exceeds it.  The rule is the project's own:
//   store        a descriptor and a ring key per archived frame (its corner, surf and outlier clouds through rl_bin, unchanged), row
//                slot * max_keyframes + frame; built lazily: a search first describes frames [described, nf) of the listed slots
//                (archived clouds never change once stored), so the per-scan path launches nothing new
//   query        the newest archived frame nf - 1 of a slot with no dropped frame
//   eligible     frame i < nf - 1 with stamp[nf - 1] - stamp[i] > lc_min_time_gap (lc_detect's comparison) and, when max_jump > 0, the
//                f32 squared distance ((dx dx) + dy dy) + dz dz of key poses i and nf - 1 < (float)(max_jump max_jump); a predicate
//                per frame, not a prefix (alego_map_set_stamps)
//   candidates   the n_cand eligible frames smallest in (D_i, i), D_i and s_i as reloc_math.h's MATCH: exactly the brute force over
//                all eligible frames and all 60 shifts, with the ring-key bound and without; those with D_i > max_dist > 0 are dropped
//   verify       candidate v in round v, the first accepted ends the slot (loop_rounds): la_plan plans every attempt on the device, source =
//                frame nf - 1 (surf, corner, outlier) under guess6 = key pose i with yaw rl_guess_yaw(yaw_i, s_i); target = frames
//                [i - lc_search_num, i + lc_search_num] within [0, nf - 2] (lc_window) under their archived poses through VoxelGrid(lc_leaf);
//                the gather is alego_loop_search's (loop_archive_gather), ICP and fitness are loop_attempts'; accepted when converged &&
//                fitness <= fitness_max
//   result       an alego_loop_result: t_correct / between = alego_loop_constraint(icp_final, guess6, key pose i); correction = the WORLD
//                correction t_correct * matrix(key pose nf - 1)^-1 (f64 rigid inverse and product, rounded to f32)
//
// alego_map_align asks the same descriptors which rigid transform takes one slot's archive into the frame of another's.
// The rule is the project's own, for a pair (src, dst) with ns and nd archived frames and none dropped:
//   queries      Q = min(n_queries, ns) source frames, query q = frame ((2 q + 1) ns) / (2 Q) (align_math.h)
//   search       every query over ALL nd destination frames (qrow in the source slot's rows, base / n the destination's): no eligibility but
//                "a query whose ring key is all zero has no candidate" (ma_mask); the n_cand smallest in (D, id), cut at max_dist > 0
//   verify       per query, candidate v in round v, the first accepted ends the query (loop_rounds over (pair, query) entries): ma_plan plans
//                every attempt on the device, source = source frame f under guess6 = destination key pose i with yaw rl_guess_yaw(yaw_i, s_i)
//                (LcDet.src1 names the source's slot; lc_gather reads it), target = destination frames lc_window(i, lc_search_num, nd - 1)
//   hypothesis   T = t_correct * matrix(source key pose f)^-1 (la_world_correction, as the appearance search's world correction)
//   consensus    ma_consensus: one wavefront per pair, one lane per hypothesis; agreement, support and the best one are align_math.h's
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "align_math.h"
#include "merge_math.h"
#include "dev_common.h"
#include "dev_cost.h"
#include "dev_copy.h"
#include "dev_mem.h"
#include "kf_store.h"
#include "loop_ctx.h"
#include "pg_math.h"
#include "prof.h"
#include "reloc.h"
#include "reloc_math.h"
#include "wave.h"

#define RL_T 256
#define RL_WAVES (RL_T / 64)
#define RL_SEARCH_BLOCKS 64        // workgroups per query of rl_search at most
#ifndef RL_BUDGET_DEFAULT
#define RL_BUDGET_DEFAULT (1 << 22)   // (query, frame) pairs per chunk of the search: 12 B of scratch each
#endif
static_assert(RL_NR % 4 == 0 && RL_SW == 5, "a sector is five words: the lanes of rl_search stride 5 words");

// one record per listed slot, written by rl_desc (mode 1): what the host needs of the slot's state
struct RlSlot {
  int frame, n[KF_KINDS];   // LI_FRAME; points of laser_corner_ds_, laser_surf_ds_, laser_outlier_ds_ (clamped to their capacities)
  double t_m2l[3], q_m2l[4];
};

// one record per query of the search kernels; off is filled in by rl_search_run
struct RlQuery {
  int qrow;        // row of qdesc / qkey
  int base, n;     // searched in rows base .. base + n - 1 of mdesc / mkey; list entries and candidate ids are 0 .. n - 1
  int off;         // where the query's n-wide rows of bound / list2 / res2 start
  int tag, pad[3]; // the caller's (appearance search: the slot)
};
#define RL_ERR "descriptor search: "   // prefix of an allocation's error
#define RL_INELIGIBLE 0xFFFFFFFFu   // a bound no frame reaches (B <= 20 * 15300): rl_pick and rl_list2 pass such a frame over

// ---- descriptors ----------------------------------------------------------------------------------------------------------------------
// mode 0: frame blockIdx.x of the map store -> desc / key row blockIdx.x; mode 1: the current scan of slot list[blockIdx.x] -> row `slot`,
// and for the host the slot's record state[blockIdx.x] and a copy of its ring key klist[blockIdx.x]; mode 2: archived frame list[2 b + 1] of
// slot list[2 b] (b = blockIdx.x; one contiguous run of the archive) -> row slot * arc_frames_cap + frame
// the finished tile of a workgroup -> row `row` of desc / key; returns ring tid's key (tid < RL_NR)
DEV_INLINE int rl_desc_store(const int* s_bin, uint32_t* desc, uint16_t* key, size_t row, int tid) {
  uint32_t* d = desc + row * RL_WORDS;
  for (int i = tid; i < RL_WORDS; i += RL_T)
    d[i] = (uint32_t)s_bin[4 * i] | ((uint32_t)s_bin[4 * i + 1] << 8) | ((uint32_t)s_bin[4 * i + 2] << 16) | ((uint32_t)s_bin[4 * i + 3] << 24);
  int s = 0;
  if (tid < RL_NR) {
    for (int c = 0; c < RL_NS; ++c) s += s_bin[c * RL_NR + tid];
    key[row * RL_NR + tid] = (uint16_t)s;
  }
  return s;
}
__global__ void __launch_bounds__(RL_T) rl_desc(LmCtx L, int mode, const int* list, float w, float zoff, uint32_t* desc, uint16_t* key, RlSlot* state, uint16_t* klist) {
  __shared__ int s_bin[RL_BYTES];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int i = tid; i < RL_BYTES; i += RL_T) s_bin[i] = 0;
  __syncthreads();
  const int e = mode == 0 ? b : list[mode == 1 ? b : 2 * b];   // map frame / slot
  KfClouds C;
  size_t row = (size_t)e;
  if (mode == 0) C = kf_clouds_row_at(L, 0, e);
  else if (mode == 1) C = kf_clouds_cur(L, e);
  else { const int f = list[2 * b + 1]; C = kf_clouds(kf_arc_frame(L, e, f)); row = arc_row(L, e, f); }
#pragma unroll
  for (int kind = 0; kind < KF_KINDS; ++kind)
    for (int i = tid; i < C.n[kind]; i += RL_T) {
      const float4 p = C.pts[kind][i];
      int bin, code;
      if (rl_bin(p.x, p.y, p.z, w, zoff, &bin, &code)) atomicMax(&s_bin[bin], code);
    }
  __syncthreads();
  const int s = rl_desc_store(s_bin, desc, key, row, tid);
  if (mode == 1 && tid < RL_NR) klist[(size_t)b * RL_NR + tid] = (uint16_t)s;
  if (mode == 1 && tid == 0) {
    const double* ld = L.ld + (size_t)e * LD_COUNT;
    RlSlot S;
    S.frame = L.li[(size_t)e * LI_COUNT + LI_FRAME];
    for (int k = 0; k < KF_KINDS; ++k) S.n[k] = C.n[k];
    for (int k = 0; k < 3; ++k) S.t_m2l[k] = ld[LD_T_M2L + k];
    for (int k = 0; k < 4; ++k) S.q_m2l[k] = ld[LD_Q_M2L + k];
    state[b] = S;
  }
}

// ring keys of descriptors handed in by the host (alego_debug_reloc_search): one workgroup of 64 per descriptor
__global__ void __launch_bounds__(64) rl_keys(const uint32_t* desc, uint16_t* key) {
  const uint8_t* d = (const uint8_t*)(desc + (size_t)blockIdx.x * RL_WORDS);
  if (threadIdx.x < RL_NR) {
    int s = 0;
    for (int c = 0; c < RL_NS; ++c) s += d[c * RL_NR + threadIdx.x];
    key[(size_t)blockIdx.x * RL_NR + threadIdx.x] = (uint16_t)s;
  }
}

// ---- the search -------------------------------------------------------------------------------------------------------------------------
// Queries of a chunk are numbered q = 0 .. nq - 1 and described by qr[q] (RlQuery).
// grid (ceil(largest n / RL_T), nq)
__global__ void __launch_bounds__(RL_T) rl_bound(const RlQuery* qr, const uint16_t* qkey, const uint16_t* mkey, uint32_t* bound) {
  const RlQuery Q = qr[blockIdx.y];
  const int i = blockIdx.x * RL_T + threadIdx.x;
  if (i >= Q.n) return;
  bound[(size_t)Q.off + i] = rl_key_bound(qkey + (size_t)Q.qrow * RL_NR, mkey + ((size_t)Q.base + i) * RL_NR);
}

// does a ring key hold anything?  (every code is >= 1: an all-zero key is a frame with no point in range)
DEV_INLINE bool rl_key_any(const uint16_t* k) {
  int any = 0;
#pragma unroll
  for (int r = 0; r < RL_NR; ++r) any |= k[r];
  return any != 0;
}

// Eligibility of the appearance search (the header comment's rule); grid as rl_bound.  Query q is the newest archived frame Q.n of slot
// Q.tag, frame i < Q.n a frame of the same slot.  A query whose ring key is all zero (no point in range: every code is >= 1) has no
// eligible frame.  nelig[q] += the eligible frames (a sum of integers does not depend on the order; zeroed by the host).
__global__ void __launch_bounds__(RL_T) la_elig(LmCtx L, const RlQuery* qr, const uint16_t* key, double min_time_gap, float jump2, uint32_t* bound, int* nelig) {
  const RlQuery Q = qr[blockIdx.y];
  const int i = blockIdx.x * RL_T + threadIdx.x;
  bool el = false;
  if (i < Q.n) {
    const size_t fb = arc_row(L, Q.tag, 0);
    el = rl_key_any(key + (size_t)Q.qrow * RL_NR) && L.arc_stamp[fb + Q.n] - L.arc_stamp[fb + i] > min_time_gap;   // lc_detect's comparison (:782)
    if (jump2 >= 0.f) {
      const float *a = arc_pose_of(L, Q.tag, i), *b = arc_pose_of(L, Q.tag, Q.n);
      const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
      el = el && ((dx * dx) + dy * dy) + dz * dz < jump2;
    }
    if (!el) bound[(size_t)Q.off + i] = RL_INELIGIBLE;
  }
  const int c = __popcll(__ballot(el));
  if (c && lane_id() == 0) atomicAdd(&nelig[blockIdx.y], c);
}

// grid (nq): listA[q][0 .. cntA[q]) = the min(n_cand, eligible) eligible frames smallest in (B, id), by rounds of "smallest key above the last one"
__global__ void __launch_bounds__(RL_T) rl_pick(const RlQuery* qr, const uint32_t* bound, int n_cand, int* listA, int* cntA) {
  __shared__ unsigned long long s_min[RL_WAVES];
  const int q = blockIdx.x, tid = threadIdx.x;
  const RlQuery Q = qr[q];
  const uint32_t* b = bound + (size_t)Q.off;
  const int N = Q.n;
  unsigned long long last = 0ull;
  int r = 0;
  for (; r < min(n_cand, N); ++r) {
    unsigned long long best = ~0ull;
    for (int i = tid; i < N; i += RL_T) {
      const unsigned long long key = ((unsigned long long)b[i] << 32) | (uint32_t)i;
      if (b[i] != RL_INELIGIBLE && (r == 0 || key > last)) best = min(best, key);
    }
    last = block_min_u64<RL_WAVES>(best, s_min);
    if (last == ~0ull) break;   // (the same value in every thread) no eligible frame is left
    if (tid == 0) listA[q * ALEGO_RELOC_MAX_CAND + r] = (int)(last & 0xffffffffu);
  }
  if (tid == 0) cntA[q] = r;
}

// grid (workgroups per query, nq): res[o + j] = D << 8 | s of frame list[o + j], j < cnt[q]; o = q * stride, or the query's Q.off when stride == 0
__global__ void __launch_bounds__(RL_T) rl_search(const RlQuery* qr, const uint32_t* qdesc, const uint32_t* __restrict__ mdesc, const int* list, const int* cnt, int stride,
                                                  uint32_t* res) {
  __shared__ uint32_t s_q[2 * RL_WORDS];
  const int q = blockIdx.y, tid = threadIdx.x;
  const RlQuery Q = qr[q];
  const uint32_t* qd = qdesc + (size_t)Q.qrow * RL_WORDS;
  for (int i = tid; i < 2 * RL_WORDS; i += RL_T) s_q[i] = qd[i < RL_WORDS ? i : i - RL_WORDS];
  __syncthreads();
  const int n = cnt[q];
  const size_t o = stride ? (size_t)q * stride : (size_t)Q.off;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t* col = s_q + (lane < RL_NS ? lane : 0) * RL_SW;   // (lanes 60 .. 63 repeat shift 0 and are left out of the arg-min)
  for (int j = blockIdx.x * RL_WAVES + wave; j < n; j += gridDim.x * RL_WAVES) {
    const int f = __builtin_amdgcn_readfirstlane(list[o + j]);
    const uint32_t* m = mdesc + ((size_t)Q.base + f) * RL_WORDS;
    uint32_t acc = 0;
#pragma unroll 4
    for (int c = 0; c < RL_NS; ++c) {
#pragma unroll
      for (int k = 0; k < RL_SW; ++k) acc = __builtin_amdgcn_sad_u8(col[c * RL_SW + k], m[c * RL_SW + k], acc);
    }
    const uint32_t best = wave_min_u32(lane < RL_NS ? (acc << 8) | (uint32_t)lane : 0xFFFFFFFFu);
    if (lane == 0) res[o + j] = best;
  }
}

// grid (nq): list2[q][0 .. cnt2[q]) = every eligible frame with B <= tau in id order; tau = the largest D of the first round (brute: every eligible frame)
__global__ void __launch_bounds__(RL_T) rl_list2(const RlQuery* qr, const uint32_t* bound, const uint32_t* resA, const int* cntA, int brute, int* list2, int* cnt2) {
  __shared__ int s_w[RL_WAVES];
  const int q = blockIdx.x, tid = threadIdx.x;
  const RlQuery Q = qr[q];
  const int N = Q.n;
  uint32_t tau = 0;
  for (int j = 0; j < cntA[q]; ++j) tau = max(tau, resA[q * ALEGO_RELOC_MAX_CAND + j] >> 8);
  if (brute) tau = 0xFFFFFFFFu;
  const uint32_t* b = bound + (size_t)Q.off;
  int carry = 0;
  for (int i0 = 0; i0 < N; i0 += RL_T) {
    const int i = i0 + tid;
    const int sel = (i < N && b[i] != RL_INELIGIBLE && b[i] <= tau) ? 1 : 0;
    int tot;
    const int ex = carry + block_excl_scan<RL_WAVES>(sel, s_w, &tot);
    if (sel) list2[(size_t)Q.off + ex] = i;
    carry += tot;
  }
  if (tid == 0) cnt2[q] = carry;
}

// grid (nq): the n_cand smallest (D, id) of the second list -> cand[q][r] = the candidate word (reloc_math.h; RL_CAND_NONE: none)
__global__ void __launch_bounds__(RL_T) rl_topk(const RlQuery* qr, const int* list2, const int* cnt2, const uint32_t* res2, int n_cand, unsigned long long* cand) {
  __shared__ unsigned long long s_min[RL_WAVES];
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)qr[q].off;
  const int n = cnt2[q];
  unsigned long long last = 0ull;
  for (int r = 0; r < n_cand; ++r) {
    unsigned long long best = ~0ull;
    if (r < n)
      for (int j = tid; j < n; j += RL_T) {
        const uint32_t v = res2[o + j];
        const unsigned long long key = rl_cand_pack(v >> 8, (uint32_t)list2[o + j], v & 0xffu);
        if (r == 0 || key > last) best = min(best, key);
      }
    last = block_min_u64<RL_WAVES>(best, s_min);
    if (tid == 0) cand[q * ALEGO_RELOC_MAX_CAND + r] = r < n ? last : RL_CAND_NONE;
  }
}

// ---- verification ---------------------------------------------------------------------------------------------------------------------
// grid (1 + frames, jobs): x = 0 the source — the slot's current scan under the guess (det.pose_latest); x = 1 + k the map frame jlo + k under
// its key pose; both read out surf, corner, outlier (as lc_gather reads an archived frame)
__global__ void __launch_bounds__(RL_T) rl_gather(LmCtx L, const LcJob* jobs, const LcDet* det, float4* src, float4* raw) {
  const LcJob J = jobs[blockIdx.y];
  const LcDet& D = det[J.li];
  float m[3][4];
  if (blockIdx.x == 0) {
    keypose_matrix(D.pose_latest, m);
    kf_clouds_write<RL_T>(kf_clouds_cur(L, J.slot), m, src + J.src_off);
    return;
  }
  const int f = D.jlo + (int)blockIdx.x - 1;
  if (f > D.jhi) return;
  keypose_matrix(kf_pose_of(L, kf_row_at(L, J.slot, f)), m);
  kf_clouds_write<RL_T>(kf_clouds_row_at(L, J.slot, f), m, lc_frame_out(raw, J, D, f, [&](int j) { return kf_clouds_points(kf_clouds_row_at(L, J.slot, j)); }));
}

// ---- the appearance search of a SLAM handle: planning ---------------------------------------------------------------------------------
// one thread per (listed entry e, candidate k): det[e * ALEGO_RELOC_MAX_CAND + k] = the attempt on candidate k as loop_attempts takes it
// (status 0: no such candidate), latest[e] = the key pose of the newest frame
__global__ void __launch_bounds__(64) la_plan(LmCtx L, const int* list, const unsigned long long* cand, int n, int search_num, LcDet* det, float* latest) {
  const int idx = blockIdx.x * 64 + threadIdx.x, e = idx / ALEGO_RELOC_MAX_CAND, k = idx % ALEGO_RELOC_MAX_CAND;
  if (e >= n) return;
  const int slot = list[e], nf = arc_stat_of(L, slot)[AS_FRAMES];
  if (k == 0)
    for (int j = 0; j < 6; ++j) latest[e * 6 + j] = nf > 0 ? arc_pose_of(L, slot, nf - 1)[j] : 0.f;
  LcDet D;
  memset(&D, 0, sizeof(D));
  const unsigned long long c = cand[idx];
  if (c != RL_CAND_NONE && nf >= 2) {
    D.status = 1; D.latest = nf - 1; D.closest = rl_cand_id(c);
    lc_window(D.closest, search_num, nf - 2, &D.jlo, &D.jhi);   // as lc_detect
    for (int j = 0; j < 6; ++j) D.pose_latest[j] = D.pose_closest[j] = arc_pose_of(L, slot, D.closest)[j];
    D.pose_latest[5] = rl_guess_yaw(D.pose_latest[5], rl_cand_shift(c));
    lc_det_sizes(L, slot, nf - 1, &D);
  }
  det[idx] = D;
}

// ---- alego_map_align: mask, planning, consensus -----------------------------------------------------------------------------------------------
struct MaEntry { int src, dst, frame, pair; };                              // one (pair, query): source frame `frame` of slot src searched in slot dst
struct MaHyp { float T[16], p[3]; int accepted; double fitness; };         // a hypothesis as ma_consensus reads it
struct MaCons { int support[MA_MAX_QUERIES], inlier[MA_MAX_QUERIES], best, pad; };   // its verdict on one pair

// grid as rl_bound: a query with an all-zero ring key has no candidate
__global__ void __launch_bounds__(RL_T) ma_mask(const RlQuery* qr, const uint16_t* key, uint32_t* bound) {
  const RlQuery Q = qr[blockIdx.y];
  const int i = blockIdx.x * RL_T + threadIdx.x;
  if (i < Q.n && !rl_key_any(key + (size_t)Q.qrow * RL_NR)) bound[(size_t)Q.off + i] = RL_INELIGIBLE;
}

// one thread per (entry e, candidate k): det[e * ALEGO_RELOC_MAX_CAND + k] = the attempt on candidate k as loop_attempts takes it (status 0: no such
// candidate) from both archives' tables, spose[e] = the source key pose of the entry
__global__ void __launch_bounds__(64) ma_plan(LmCtx L, const MaEntry* ent, const unsigned long long* cand, int n, int search_num, LcDet* det, float* spose) {
  const int idx = blockIdx.x * 64 + threadIdx.x, e = idx / ALEGO_RELOC_MAX_CAND, k = idx % ALEGO_RELOC_MAX_CAND;
  if (e >= n) return;
  const MaEntry E = ent[e];
  if (k == 0)
    for (int j = 0; j < 6; ++j) spose[e * 6 + j] = arc_pose_of(L, E.src, E.frame)[j];
  LcDet D;
  memset(&D, 0, sizeof(D));
  const unsigned long long c = cand[idx];
  if (c != RL_CAND_NONE) {
    const int nd = arc_stat_of(L, E.dst)[AS_FRAMES];
    D.status = 1; D.latest = E.frame; D.closest = rl_cand_id(c); D.src1 = E.src + 1;
    lc_window(D.closest, search_num, nd - 1, &D.jlo, &D.jhi);   // every destination frame is admissible
    for (int j = 0; j < 6; ++j) D.pose_latest[j] = D.pose_closest[j] = arc_pose_of(L, E.dst, D.closest)[j];
    D.pose_latest[5] = rl_guess_yaw(D.pose_latest[5], rl_cand_shift(c));
    lc_det_sizes(L, E.dst, E.frame, &D);
  }
  det[idx] = D;
}

// grid (pairs), one wavefront each, lane b = hypothesis b of the pair (nq[pair] <= 32 of them).  Hypothesis a is wave-uniform (scalar loads) in
// round a: lane b tests AGREE(a, b), the wavefront's sum is support(a).  Then the arg-best in three uniform steps (align_math.h's order) and the
// inliers: one more test per lane.  No LDS, no atomics.
__global__ void __launch_bounds__(64) ma_consensus(const MaHyp* hyp, const int* nq, double tol_trans, double tol_rot, MaCons* out) {
  const int lane = lane_id(), n = nq[blockIdx.x];
  const MaHyp* H = hyp + (size_t)blockIdx.x * MA_MAX_QUERIES;
  MaHyp B;
  memset(&B, 0, sizeof(B));
  if (lane < n) B = H[lane];
  const bool mine = lane < n && B.accepted != 0;
  int support = 0;
  for (int a = 0; a < n; ++a) {
    const int ag = (H[a].accepted && mine && ma_agree(H[a].T, H[a].p, B.T, B.p, tol_trans, tol_rot)) ? 1 : 0;
    const int s = wave_sum_i32(ag);
    if (lane == a) support = s;
  }
  const bool in = mine && support >= 1;
  const uint32_t smax = wave_max_u32(in ? (uint32_t)support : 0u);
  const bool top = in && (uint32_t)support == smax;
  const unsigned long long key = ma_fit_key(B.fitness);
  const unsigned long long kmin = wave_min_u64(top ? key : ~0ull);
  const uint32_t bl = wave_min_u32(top && key == kmin ? (uint32_t)lane : 0xFFFFFFFFu);
  const int best = smax == 0u ? -1 : (int)bl;
  MaCons* O = out + blockIdx.x;
  if (lane < MA_MAX_QUERIES) {
    O->support[lane] = support;
    O->inlier[lane] = (best >= 0 && mine && ma_agree(H[best].T, H[best].p, B.T, B.p, tol_trans, tol_rot)) ? 1 : 0;
  }
  if (lane == 0) { O->best = best; O->pad = 0; }
}

struct RlApply { int slot, pad; double rc[12], params6[6]; };
// one lane per accepted slot: correctPoses :579-580 on map -> odom exactly as lm_apply_correction computes it, then params_
__global__ void __launch_bounds__(64) rl_apply(LmCtx L, const RlApply* a, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double* ld = L.ld + (size_t)a[i].slot * LD_COUNT;
  dq_apply_correction<double, true>(ld + LD_Q_M2O, ld + LD_T_M2O, a[i].rc);
#pragma unroll
  for (int k = 0; k < 6; ++k) ld[LD_PARAMS + k] = a[i].params6[k];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
struct RlCtx {
  int N = 0, n_slots = 0;
  float w = 0.f, zoff = 0.f;
  uint32_t *mdesc = nullptr, *qdesc = nullptr;
  uint16_t *mkey = nullptr, *qkey = nullptr;
  int* list = nullptr;                  // [n_slots] the listed slots of a call
  RlSlot* state = nullptr;              // [n_slots] their records (rl_desc)
  uint16_t* klist = nullptr;            // [n_slots][RL_NR] their ring keys, in list order
  RlApply* apply = nullptr;             // [n_slots]
  std::vector<int> cnt;                 // host copy of the store: points per frame
  std::vector<float> pose;              // [N][6]
  // search scratch, grown on first use
  long long budget = RL_BUDGET_DEFAULT;
  int brute = 0;
  size_t pairs_cap = 0, q_cap = 0;
  uint32_t *bound = nullptr, *res2 = nullptr, *resA = nullptr;
  int *list2 = nullptr, *cnt2 = nullptr, *listA = nullptr, *cntA = nullptr, *nelig = nullptr;
  RlQuery* qr = nullptr;
  unsigned long long* cand = nullptr;
  int stats[2] = {0, 0};                // of the last search: (query, frame) pairs the second round evaluated, pairs in all
  // the appearance search of a SLAM handle (alego_loop_appearance_enable; la_cap == 0: off, nothing of it is allocated)
  int la_slots = 0, la_cap = 0;         // slots; rows per slot (max_keyframes of the archive)
  float la_w = 0.f, la_zoff = 0.f;
  uint32_t* la_desc = nullptr;          // [la_slots][la_cap][RL_WORDS] descriptor of archived frame f of slot s at row s * la_cap + f
  uint16_t* la_key = nullptr;           // [la_slots][la_cap][RL_NR]
  std::vector<int> la_described;        // [la_slots] frames described so far: rows [0, la_described) of the slot are valid
  int* la_list = nullptr;               // [la_slots] the listed slots of a call
  unsigned long long* la_cand = nullptr;   // [la_slots][ALEGO_RELOC_MAX_CAND] their candidates
  LcDet* la_det = nullptr;              // [la_slots][ALEGO_RELOC_MAX_CAND] the attempts la_plan planned
  float* la_latest = nullptr;           // [la_slots][6] key pose of the newest frame
  // alego_map_align: grown by the calls and kept
  DevBuf<MaEntry> ma_ent;
  DevBuf<unsigned long long> ma_cand;   // [entries][ALEGO_RELOC_MAX_CAND]
  DevBuf<LcDet> ma_det;                 // [entries][ALEGO_RELOC_MAX_CAND]
  DevBuf<float> ma_spose;               // [entries][6]
  DevBuf<MaHyp> ma_hyp;                 // [pairs][MA_MAX_QUERIES]
  DevBuf<int> ma_nq;                    // [pairs]
  DevBuf<MaCons> ma_cons;               // [pairs]
  DevBuf<int> la_pend;                  // (slot, frame) pairs still to describe
  DevPool la_store;                     // owns the la_* arrays above (valid while la_cap > 0)
  DevPool store, scratch;               // own what reloc_enable allocates (valid while n_slots > 0) and the search scratch (valid while pairs_cap > 0)
};

void reloc_ctx_destroy(RlCtx* R) {
  if (!R) return;
  R->scratch.clear(); R->store.clear(); R->la_store.clear(); R->la_pend.clear();
  R->ma_ent.clear(); R->ma_cand.clear(); R->ma_det.clear(); R->ma_spose.clear(); R->ma_hyp.clear(); R->ma_nq.clear(); R->ma_cons.clear();
  delete R;
}
void reloc_ctx_set(RlCtx** pr, int what, long long v) {   // what 0: pairs per chunk of the search, 1: brute force
  if (!*pr) *pr = new RlCtx();
  if (what == 0) (*pr)->budget = std::max(1LL, v); else (*pr)->brute = v != 0;
}
bool reloc_enabled(const RlCtx* R) { return R && R->n_slots > 0; }

// descriptors and ring keys of the store's L.loc_n frames (queued on st, finished on return), and the host copy of their counts and poses
static void rl_describe_map(RlCtx* R, const LmCtx& L, hipStream_t st, DevTry* c) {
  const int N = L.loc_n;
  if (N > 0) ALEGO_LAUNCH(rl_desc, dim3(N), dim3(RL_T), 0, st, L, 0, (const int*)nullptr, R->w, R->zoff, R->mdesc, R->mkey, (RlSlot*)nullptr, (uint16_t*)nullptr);
  std::vector<int> cnt((size_t)N * KF_CNT_W);
  std::vector<float> pose((size_t)N * KF_POSE_W);
  if (c->down(cnt, kf_cnt_of(L, kf_row_at(L, 0, 0)), st).down(pose, kf_pose_of(L, kf_row_at(L, 0, 0)), st).wait(st)) return;
  R->cnt.resize(N); R->pose.resize((size_t)N * 6);
  for (int i = 0; i < N; ++i) {
    R->cnt[i] = kf_clouds_points(kf_clouds_row_at(L, 0, i, cnt.data() + (size_t)i * KF_CNT_W));   // as rl_gather counts them
    for (int k = 0; k < 6; ++k) R->pose[(size_t)i * 6 + k] = pose[(size_t)i * KF_POSE_W + k];
  }
  R->N = N;
}

int reloc_enable(RlCtx** pr, const LmCtx& L, int n_slots, double max_range, double z_offset, hipStream_t st, std::string* err) {
  if (!*pr) *pr = new RlCtx();
  RlCtx* R = *pr;
  const size_t F = (size_t)std::max(L.fr_mod, L.loc_n);   // the store's capacity: alego_loc_update_from_map may hand it up to that many frames
  R->w = rl_ring_width(max_range); R->zoff = rl_z_offset(z_offset);
  auto undo = [&](int rc) { R->store.clear(); return rc; };   // (the handle stays what it was)
  const DevGet get{R->store, RL_ERR, err};
  if (!get(&R->mdesc, F * RL_WORDS) || !get(&R->mkey, F * RL_NR) || !get(&R->qdesc, (size_t)n_slots * RL_WORDS) || !get(&R->qkey, (size_t)n_slots * RL_NR) ||
      !get(&R->list, (size_t)n_slots) || !get(&R->apply, (size_t)n_slots) || !get(&R->state, (size_t)n_slots) || !get(&R->klist, (size_t)n_slots * RL_NR)) return undo(ALEGO_ERR_HIP);
  DevTry c("alego_reloc_enable", err);
  c.took(hipMemsetAsync(R->qdesc, 0, std::max<size_t>(16, (size_t)n_slots * RL_BYTES), st), "clearing");
  if (c.ok()) c.took(hipMemsetAsync(R->qkey, 0, std::max<size_t>(16, (size_t)n_slots * RL_NR * 2), st), "clearing");
  if (c.ok()) rl_describe_map(R, L, st, &c);
  if (c) return undo(c);
  R->n_slots = n_slots;
  return 0;
}
// the store changed (alego_loc_update_from_map): the descriptors and ring keys of its frames are built again; a failure leaves none (no frame is a candidate)
int reloc_refresh(RlCtx* R, const LmCtx& L, hipStream_t st, std::string* err) {
  if (!reloc_enabled(R)) return 0;
  DevTry c("alego_loc_update_from_map", err, "describing the map");
  rl_describe_map(R, L, st, &c);
  if (c) { R->N = 0; R->cnt.clear(); R->pose.clear(); }
  return c;
}

// The exact search of nq queries (qr[q]; off is filled in here): cand[q][r] = the candidate word, RL_CAND_NONE where fewer frames are eligible.
// Queries are taken in chunks of consecutive queries whose frames sum to at most the budget; a query's result does not depend on its chunk.
// mask (may be empty) runs behind rl_bound on the records and bounds of a chunk of c queries whose largest n is nmax; nelig (may be
// null) receives what it summed into R->nelig per query.
typedef std::function<void(const RlQuery* qr, int c, int nmax, uint32_t* bound, int* nelig, hipStream_t st)> RlMask;
static int rl_search_run(RlCtx* R, const uint32_t* qdesc, const uint16_t* qkey, RlQuery* qr, int nq, const uint32_t* mdesc, const uint16_t* mkey, int n_cand,
                         unsigned long long* cand, const RlMask& mask, int* nelig, hipStream_t st, std::string* err) {
  for (size_t i = 0; i < (size_t)nq * ALEGO_RELOC_MAX_CAND; ++i) cand[i] = RL_CAND_NONE;
  long long all = 0;
  for (int q = 0; q < nq; ++q) { all += qr[q].n; if (nelig) nelig[q] = 0; }
  R->stats[0] = 0; R->stats[1] = (int)std::min<long long>(all, 0x7fffffff);
  if (nq == 0 || all == 0) return 0;
  DevTry t("descriptor search", err);
  // chunks [first, first + count): consecutive queries; pairs and queries of the largest chunk size the scratch
  const long long budget = std::min<long long>(R->budget, 1LL << 30);
  std::vector<std::pair<int, int>> chunks;
  size_t pc = 1, qc = 1;
  for (int q0 = 0; q0 < nq;) {
    long long sum = 0;
    int c = 0;
    while (q0 + c < nq && (c == 0 || sum + qr[q0 + c].n <= budget)) { qr[q0 + c].off = (int)sum; sum += qr[q0 + c].n; ++c; }
    if (sum > 0x7fffffffLL) { *err = "descriptor search: a query's map is too large"; return ALEGO_ERR_ARG; }
    chunks.emplace_back(q0, c);
    pc = std::max(pc, (size_t)sum); qc = std::max(qc, (size_t)c);
    q0 += c;
  }
  if (R->pairs_cap < pc || R->q_cap < qc) {
    pc = std::max(R->pairs_cap, pc); qc = std::max(R->q_cap, qc);
    if (t.wait(st)) return t;
    R->scratch.clear(); R->pairs_cap = R->q_cap = 0;
    const DevGet get{R->scratch, RL_ERR, err};
    if (!get(&R->bound, pc) || !get(&R->res2, pc) || !get(&R->list2, pc) || !get(&R->resA, qc * ALEGO_RELOC_MAX_CAND) || !get(&R->listA, qc * ALEGO_RELOC_MAX_CAND) || !get(&R->cntA, qc) ||
        !get(&R->cnt2, qc) || !get(&R->qr, qc) || !get(&R->nelig, qc) || !get(&R->cand, qc * ALEGO_RELOC_MAX_CAND)) { R->scratch.clear(); return ALEGO_ERR_HIP; }
    R->pairs_cap = pc; R->q_cap = qc;
  }
  std::vector<int> cnt2;
  for (const auto& ch : chunks) {
    const int q0 = ch.first, c = ch.second;
    int nmax = 0;
    for (int q = q0; q < q0 + c; ++q) nmax = std::max(nmax, qr[q].n);
    const int nblk = std::max(1, std::min(RL_SEARCH_BLOCKS, (nmax + RL_WAVES - 1) / RL_WAVES));
    const dim3 gb(std::max(1, (nmax + RL_T - 1) / RL_T), c);
    if (t.at("upload").up(R->qr, qr + q0, (size_t)c, st)) return t;
    ALEGO_LAUNCH(rl_bound, gb, dim3(RL_T), 0, st, (const RlQuery*)R->qr, qkey, mkey, R->bound);
    if (mask) {
      if (t.took(hipMemsetAsync(R->nelig, 0, (size_t)c * sizeof(int), st), "the search")) return t;
      mask(R->qr, c, nmax, R->bound, R->nelig, st);
    }
    ALEGO_LAUNCH(rl_pick, dim3(c), dim3(RL_T), 0, st, (const RlQuery*)R->qr, R->bound, n_cand, R->listA, R->cntA);
    ALEGO_LAUNCH(rl_search, dim3(1, c), dim3(RL_T), 0, st, (const RlQuery*)R->qr, qdesc, mdesc, R->listA, R->cntA, ALEGO_RELOC_MAX_CAND, R->resA);
    ALEGO_LAUNCH(rl_list2, dim3(c), dim3(RL_T), 0, st, (const RlQuery*)R->qr, R->bound, R->resA, R->cntA, R->brute, R->list2, R->cnt2);
    ALEGO_LAUNCH(rl_search, dim3(nblk, c), dim3(RL_T), 0, st, (const RlQuery*)R->qr, qdesc, mdesc, R->list2, R->cnt2, 0, R->res2);
    ALEGO_LAUNCH(rl_topk, dim3(c), dim3(RL_T), 0, st, (const RlQuery*)R->qr, R->list2, R->cnt2, R->res2, n_cand, R->cand);
    // (the next chunk reuses the scratch: copies and kernels are ordered on `st`; cand is pageable, so the copy below has left the device when it returns)
    cnt2.resize((size_t)c);
    t.at("the search").down(cand + (size_t)q0 * ALEGO_RELOC_MAX_CAND, R->cand, (size_t)c * ALEGO_RELOC_MAX_CAND, st).down(cnt2, R->cnt2, st);
    if (mask && nelig) t.down(nelig + q0, R->nelig, (size_t)c, st);
    if (t.wait(st)) return t;
    for (int v : cnt2) R->stats[0] = (int)std::min<long long>((long long)R->stats[0] + v, 0x7fffffff);
  }
  return 0;
}
// every query in rows 0 .. N - 1 of one map: query q is row sel[q]
static std::vector<RlQuery> rl_whole_map(const int* sel, int nq, int N) {
  std::vector<RlQuery> qr((size_t)nq);
  for (int q = 0; q < nq; ++q) { std::memset(&qr[q], 0, sizeof(RlQuery)); qr[q].qrow = sel[q]; qr[q].n = N; }
  return qr;
}

void reloc_debug_stats(const RlCtx* R, int out[2]) { out[0] = R ? R->stats[0] : 0; out[1] = R ? R->stats[1] : 0; }

int reloc_debug_search(RlCtx** pr, const uint8_t* map_desc, int n_map, const uint8_t* q_desc, int n_q, int n_cand, int32_t* ids, int32_t* dists, int32_t* shifts,
                       hipStream_t st, std::string* err) {
  if (!*pr) *pr = new RlCtx();
  RlCtx* R = *pr;
  DevPool tmp;   // temporaries of this call
  uint32_t *md = nullptr, *qd = nullptr;
  uint16_t *mk = nullptr, *qk = nullptr;
  const DevGet get{tmp, RL_ERR, err};
  if (!get(&md, (size_t)n_map * RL_WORDS) || !get(&qd, (size_t)n_q * RL_WORDS) || !get(&mk, (size_t)n_map * RL_NR) || !get(&qk, (size_t)n_q * RL_NR)) return ALEGO_ERR_HIP;
  DevTry c("debug_reloc_search", err);   // (a descriptor: RL_BYTES bytes on the host, RL_WORDS words on the device)
  if (c.up(reinterpret_cast<uint8_t*>(md), map_desc, (size_t)n_map * RL_BYTES, st).up(reinterpret_cast<uint8_t*>(qd), q_desc, (size_t)n_q * RL_BYTES, st)) return c;
  if (n_map) ALEGO_LAUNCH(rl_keys, dim3(n_map), dim3(64), 0, st, md, mk);
  if (n_q) ALEGO_LAUNCH(rl_keys, dim3(n_q), dim3(64), 0, st, qd, qk);
  std::vector<int> sel((size_t)n_q);
  for (int q = 0; q < n_q; ++q) sel[q] = q;
  std::vector<unsigned long long> cand((size_t)n_q * ALEGO_RELOC_MAX_CAND);
  std::vector<RlQuery> qr = rl_whole_map(sel.data(), n_q, n_map);
  int rc = rl_search_run(R, qd, qk, qr.data(), n_q, md, mk, n_cand, cand.data(), RlMask(), nullptr, st, err);
  const hipError_t we = dev_wait(st);
  if (!rc) rc = c.took(we, "kernels");
  if (rc) return rc;
  for (int q = 0; q < n_q; ++q)
    for (int r = 0; r < n_cand; ++r) {
      const size_t o = (size_t)q * n_cand;
      if (!rl_cand_unpack(&cand[(size_t)q * ALEGO_RELOC_MAX_CAND], r, ids + o, dists + o, shifts + o)) ids[o + r] = dists[o + r] = shifts[o + r] = -1;
    }
  return 0;
}

int reloc_debug_get(RlCtx* R, int slot, const char* name, const void** src, size_t* bytes) {
  if (!reloc_enabled(R)) return ALEGO_ERR_ARG;
  const std::string s(name);
  if (s == "rl_query_desc") { *src = R->qdesc + (size_t)slot * RL_WORDS; *bytes = RL_BYTES; }
  else if (s == "rl_query_key") { *src = R->qkey + (size_t)slot * RL_NR; *bytes = RL_NR * 2; }
  else if (s == "rl_map_desc") { *src = R->mdesc; *bytes = (size_t)R->N * RL_BYTES; }
  else if (s == "rl_map_key") { *src = R->mkey; *bytes = (size_t)R->N * RL_NR * 2; }
  else return ALEGO_ERR_ARG;
  return 0;
}

// f64 arithmetic of `apply` (include/alego_mi355x.h): rc = t_map * T_cur^-1, params6 = translation and Euler angles of t_map
static void rl_placement(const float* t_map, const double* t_cur, const double* q_cur /* w x y z */, double* rc, double* params6) {
  const double w = q_cur[0], x = q_cur[1], y = q_cur[2], z = q_cur[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double Rc[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};   // dq_to_mat
  double Rm[9], tm[3];
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rm[r * 3 + c] = (double)t_map[r * 4 + c]; tm[r] = (double)t_map[r * 4 + 3]; }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) rc[r * 4 + c] = Rm[r * 3 + 0] * Rc[c * 3 + 0] + Rm[r * 3 + 1] * Rc[c * 3 + 1] + Rm[r * 3 + 2] * Rc[c * 3 + 2];   // R_map R_cur^T
  }
  for (int r = 0; r < 3; ++r) rc[r * 4 + 3] = tm[r] - (rc[r * 4 + 0] * t_cur[0] + rc[r * 4 + 1] * t_cur[1] + rc[r * 4 + 2] * t_cur[2]);
  params6[0] = tm[0]; params6[1] = tm[1]; params6[2] = tm[2];
  params6[3] = std::atan2(Rm[7], Rm[8]);
  params6[4] = std::atan2(-Rm[6], std::sqrt(Rm[7] * Rm[7] + Rm[8] * Rm[8]));
  params6[5] = std::atan2(Rm[3], Rm[0]);
}

int reloc_run(RlCtx* R, LcCtx** lc, const LmCtx& L, const alego_params& P, const int* slots, int n, int n_cand, int verify, int apply, alego_reloc_result* out,
              hipStream_t st, std::string* err) {
  const int N = R->N;
  for (int i = 0; i < n; ++i) { std::memset(&out[i], 0, sizeof(out[i])); out[i].verified = -1; }
  if (n == 0) return 0;
  // the listed slots' descriptors, and of their state what the host needs (the caller has drained every stream): O(n), whatever the handle's size
  std::vector<RlSlot> state((size_t)n);
  std::vector<uint16_t> qkey((size_t)n * RL_NR);
  DevTry c("alego_loc_relocalize", err);
  if (c.up(R->list, slots, (size_t)n, st)) return c;
  ALEGO_LAUNCH(rl_desc, dim3(n), dim3(RL_T), 0, st, L, 1, (const int*)R->list, R->w, R->zoff, R->qdesc, R->qkey, R->state, R->klist);
  if (c.at("descriptors").down(state, R->state, st).down(qkey, R->klist, st).wait(st)) return c;
  // searchable: a mapping frame has run and a point lies in range (every code is >= 1, so an all-zero key is an empty descriptor)
  std::vector<int> qi, sel;
  for (int i = 0; i < n; ++i) {
    int any = 0;
    for (int r = 0; r < RL_NR; ++r) any |= qkey[(size_t)i * RL_NR + r];
    if (state[i].frame > 0 && any && N > 0) { qi.push_back(i); sel.push_back(slots[i]); }
  }
  std::vector<unsigned long long> cand(qi.size() * ALEGO_RELOC_MAX_CAND + 1);
  std::vector<RlQuery> qr = rl_whole_map(sel.data(), (int)qi.size(), N);
  if (int rc = rl_search_run(R, R->qdesc, R->qkey, qr.data(), (int)qi.size(), R->mdesc, R->mkey, n_cand, cand.data(), RlMask(), nullptr, st, err)) return rc;
  for (size_t a = 0; a < qi.size(); ++a) {
    alego_reloc_result& r = out[qi[a]];
    while (r.n_cand < n_cand && rl_cand_unpack(&cand[a * ALEGO_RELOC_MAX_CAND], r.n_cand, r.cand_id, r.cand_dist, r.cand_shift)) ++r.n_cand;
    r.status = r.n_cand > 0 ? 1 : 0;
  }
  // verification (loop_rounds): candidate v of slot i is the scan under the guess against the map frames around the candidate
  if (int rc = loop_rounds(lc, P, R->n_slots, slots, n, verify, [&](const LcJob* jobs, const LcDet* dd, int J, int nfr, float4* src, float4* raw, hipStream_t s2) {
        ALEGO_LAUNCH(rl_gather, dim3(nfr, J), dim3(RL_T), 0, s2, L, jobs, dd, src, raw);
      }, [&](int i, int v, LcDet* D) {
        const alego_reloc_result& r = out[i];
        if (r.n_cand <= v) return false;
        const int f = r.cand_id[v];
        D->latest = -1; D->closest = f;
        lc_window(f, P.lc_search_num, N - 1, &D->jlo, &D->jhi);
        for (int k = 0; k < 6; ++k) D->pose_latest[k] = D->pose_closest[k] = R->pose[(size_t)f * 6 + k];
        D->pose_latest[5] = rl_guess_yaw(D->pose_latest[5], r.cand_shift[v]);
        D->n_src = state[i].n[KF_CORNER] + state[i].n[KF_SURF] + state[i].n[KF_OUTL];
        for (int j = D->jlo; j <= D->jhi; ++j) D->n_raw += R->cnt[j];
        return true;
      }, [&](int i, int v, const LcDet& D, const LcOut& O) {
        alego_reloc_result& r = out[i];
        r.converged = O.converged; r.iterations = O.iterations; r.n_source = O.n_source; r.n_target = O.n_target; r.fitness = O.fitness;
        for (int k = 0; k < 16; ++k) r.correction[k] = O.correction[k];
        for (int k = 0; k < 6; ++k) r.guess6[k] = D.pose_latest[k];
        double between[12];
        alego_loop_constraint(r.correction, r.guess6, r.guess6, r.t_map, between);   // t_map = correction * matrix(guess6), as t_correct (:714-715)
        if (!(O.converged && O.fitness <= P.lc_fitness_max)) return false;   // :697
        r.status = 2; r.verified = v;
        rl_placement(r.t_map, state[i].t_m2l, state[i].q_m2l, r.rc, r.params6);
        return true;
      }, st, err)) return rc;
  if (apply) {
    std::vector<RlApply> ap;
    for (int i = 0; i < n; ++i)
      if (out[i].status == 2) {
        RlApply a;
        a.slot = slots[i]; a.pad = 0;
        std::memcpy(a.rc, out[i].rc, sizeof(a.rc)); std::memcpy(a.params6, out[i].params6, sizeof(a.params6));
        ap.push_back(a);
        out[i].applied = 1;
      }
    if (!ap.empty()) {
      if (c.at("upload").up(R->apply, ap, st)) return c;
      ALEGO_LAUNCH(rl_apply, dim3(((int)ap.size() + 63) / 64), dim3(64), 0, st, L, (const RlApply*)R->apply, (int)ap.size());
      if (c.at("apply").wait(st)) return c;
    }
  }
  return 0;
}

// ---- the appearance search of a SLAM handle: host -----------------------------------------------------------------------------------------
bool loop_app_enabled(const RlCtx* R) { return R && R->la_cap > 0; }

int loop_app_enable(RlCtx** pr, const LmCtx& L, int n_slots, double max_range, double z_offset, std::string* err) {
  if (!*pr) *pr = new RlCtx();
  RlCtx* R = *pr;
  const size_t rows = (size_t)n_slots * L.arc_frames_cap, ent = (size_t)n_slots * ALEGO_RELOC_MAX_CAND;
  const DevGet get{R->la_store, RL_ERR, err};
  if (!get(&R->la_desc, rows * RL_WORDS) || !get(&R->la_key, rows * RL_NR) || !get(&R->la_list, (size_t)n_slots) || !get(&R->la_cand, ent) || !get(&R->la_det, ent) || !get(&R->la_latest, (size_t)n_slots * 6)) {
    R->la_store.clear();
    return ALEGO_ERR_HIP;
  }
  R->la_w = rl_ring_width(max_range); R->la_zoff = rl_z_offset(z_offset);
  R->la_described.assign((size_t)n_slots, 0);
  R->la_slots = n_slots; R->la_cap = L.arc_frames_cap;
  return 0;
}

void loop_app_forget(RlCtx* R, int slot, int first) {
  if (loop_app_enabled(R) && slot >= 0 && slot < R->la_slots) R->la_described[slot] = std::min(R->la_described[slot], std::max(first, 0));
}

int loop_app_debug_get(RlCtx* R, int slot, const char* name, const void** src, size_t* bytes) {
  if (!loop_app_enabled(R)) return ALEGO_ERR_ARG;
  const std::string s(name);
  const size_t row = (size_t)slot * R->la_cap, n = (size_t)R->la_described[slot];
  if (s == "la_desc") { *src = R->la_desc + row * RL_WORDS; *bytes = n * RL_BYTES; }
  else if (s == "la_key") { *src = R->la_key + row * RL_NR; *bytes = n * RL_NR * 2; }
  else return ALEGO_ERR_ARG;
  return 0;
}

// correction = t_correct * matrix(latest6)^-1: the f32 matrices widened to f64, the rigid inverse, the product rounded to f32.  The world
// correction of the appearance search (latest6 = the newest key pose) and the hypothesis of alego_map_align (latest6 = the source key pose).
static void la_world_correction(const float* t_correct, const float* latest6, float* correction) {
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float G[16];
  double unused[12];
  alego_loop_constraint(eye, latest6, latest6, G, unused);   // G = matrix(latest6) as t_correct's initial_guess is built (:680-687)
  for (int r = 0; r < 3; ++r) {
    double t = (double)t_correct[r * 4 + 3];
    for (int c = 0; c < 3; ++c) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += (double)t_correct[r * 4 + k] * (double)G[c * 4 + k];   // R_t R_g^T
      correction[r * 4 + c] = (float)v;
      t -= v * (double)G[c * 4 + 3];                                                         // t_t - R_t R_g^T t_g
    }
    correction[r * 4 + 3] = (float)t;
  }
  correction[12] = correction[13] = correction[14] = 0.f; correction[15] = 1.f;
}

// queues the descriptors of the pending (slot, frame) pairs on `st` and counts them as described
static int la_describe(RlCtx* R, const LmCtx& L, const std::vector<int>& pend, const char* who, hipStream_t st, std::string* err) {
  if (pend.empty()) return 0;
  if (int r = DevTry(who, err).took(R->la_pend.reserve(pend.size())).up(R->la_pend.p, pend, st)) return r;
  ALEGO_LAUNCH(rl_desc, dim3((unsigned)(pend.size() / 2)), dim3(RL_T), 0, st, L, 2, (const int*)R->la_pend.p, R->la_w, R->la_zoff, R->la_desc, R->la_key, (RlSlot*)nullptr, (uint16_t*)nullptr);
  // (pend is pageable: the copy has left the host buffer when the call returns; the kernel is ordered behind it on `st`)
  for (size_t k = 0; k < pend.size(); k += 2) R->la_described[pend[k]] = std::max(R->la_described[pend[k]], pend[k + 1] + 1);   // only now: the rows are queued
  return 0;
}

int loop_app_run(RlCtx* R, LcCtx** lc, const LmCtx& L, const alego_params& P, const int* slots, int n, const alego_loop_app_opts& o, alego_loop_result* out,
                 alego_loop_app_info* info, hipStream_t st, std::string* err) {
  for (int i = 0; i < n; ++i) {
    std::memset(&out[i], 0, sizeof(out[i]));
    out[i].latest_id = out[i].closest_id = -1;
    if (info) { std::memset(&info[i], 0, sizeof(info[i])); info[i].verified = -1; }
  }
  if (n == 0) return 0;
  // frames stored / dropped of every slot (the caller has drained every stream), then the descriptors of the listed slots' frames [described, nf)
  std::vector<int> stat((size_t)R->la_slots * AS_W);
  DevTry t("alego_loop_search_appearance", err, "reading the archive");
  if (t.down(stat, arc_stat_of(L, 0), st).wait(st)) return t;
  std::vector<int> pend;
  std::vector<RlQuery> qr;
  std::vector<int> qi;
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i], nf = std::min(stat[(size_t)slot * AS_W + AS_FRAMES], R->la_cap);
    out[i].latest_id = nf - 1;
    if (stat[(size_t)slot * AS_W + AS_DROPPED] > 0) { out[i].status = -1; continue; }   // the newest key frame is not in the archive
    for (int f = std::min(R->la_described[slot], nf); f < nf; ++f) { pend.push_back(slot); pend.push_back(f); }
    if (nf < 2) continue;
    RlQuery q;
    std::memset(&q, 0, sizeof(q));
    q.base = slot * R->la_cap; q.n = nf - 1; q.qrow = q.base + nf - 1; q.tag = slot;
    qr.push_back(q); qi.push_back(i);
  }
  if (int rc = la_describe(R, L, pend, "alego_loop_search_appearance", st, err)) return rc;
  // the search: every query against the older frames of its own slot
  const float jump2 = o.max_jump > 0.0 ? (float)(o.max_jump * o.max_jump) : -1.f;
  const double gap = P.lc_min_time_gap;
  std::vector<unsigned long long> cand(qr.size() * ALEGO_RELOC_MAX_CAND + 1);
  std::vector<int> nelig(qr.size() + 1);
  if (int rc = rl_search_run(R, R->la_desc, R->la_key, qr.data(), (int)qr.size(), R->la_desc, R->la_key, o.n_cand, cand.data(),
                             [&](const RlQuery* dq, int c, int nmax, uint32_t* bound, int* ne, hipStream_t s2) {
                               ALEGO_LAUNCH(la_elig, dim3(std::max(1, (nmax + RL_T - 1) / RL_T), c), dim3(RL_T), 0, s2, L, dq, (const uint16_t*)R->la_key, gap, jump2, bound, ne);
                             }, nelig.data(), st, err)) return rc;
  if (t.at("descriptors").wait(st)) return t;   // (no query: the descriptors alone)
  std::vector<unsigned long long> ecand((size_t)n * ALEGO_RELOC_MAX_CAND, RL_CAND_NONE);   // per listed entry, after the max_dist cut
  std::vector<int> ncand((size_t)n, 0);
  bool any = false;
  for (size_t a = 0; a < qi.size(); ++a) {
    const int i = qi[a];
    unsigned long long* ec = &ecand[(size_t)i * ALEGO_RELOC_MAX_CAND];
    int k = 0;
    for (; k < o.n_cand; ++k) {
      const unsigned long long c = cand[a * ALEGO_RELOC_MAX_CAND + k];
      if (c == RL_CAND_NONE || (o.max_dist > 0 && rl_cand_dist(c) > o.max_dist)) break;
      ec[k] = c;
      if (info) rl_cand_unpack(ec, k, info[i].cand_id, info[i].cand_dist, info[i].cand_shift);
    }
    ncand[i] = k;
    if (info) { info[i].n_eligible = nelig[a]; info[i].n_cand = k; }
    if (k > 0) { out[i].status = 1; out[i].closest_id = rl_cand_id(ec[0]); any = true; }
  }
  if (!any || o.verify == 0) return 0;
  // the attempts on every candidate, planned on the device from the archive's tables
  std::vector<LcDet> plan((size_t)n * ALEGO_RELOC_MAX_CAND);
  std::vector<float> latest((size_t)n * 6);
  if (t.at("upload").up(R->la_list, slots, (size_t)n, st).up(R->la_cand, ecand, st)) return t;
  ALEGO_LAUNCH(la_plan, dim3((n * ALEGO_RELOC_MAX_CAND + 63) / 64), dim3(64), 0, st, L, (const int*)R->la_list, (const unsigned long long*)R->la_cand, n, P.lc_search_num, R->la_det, R->la_latest);
  if (t.at("planning").down(plan, R->la_det, st).down(latest, R->la_latest, st).wait(st)) return t;
  const double fitness_max = o.fitness_max > 0.0 ? o.fitness_max : P.lc_fitness_max;
  return loop_rounds(lc, P, R->la_slots, slots, n, o.verify, loop_archive_gather(L), [&](int i, int v, LcDet* D) {
    if (ncand[i] <= v) return false;
    *D = plan[(size_t)i * ALEGO_RELOC_MAX_CAND + v];
    return D->status == 1;
  }, [&](int i, int v, const LcDet& D, const LcOut& O) {
    alego_loop_result& r = out[i];
    const bool ok = loop_result_fill(D, O, fitness_max, &r);
    la_world_correction(r.t_correct, latest.data() + (size_t)i * 6, r.correction);
    if (info) {
      for (int k = 0; k < 6; ++k) info[i].guess6[k] = D.pose_latest[k];
      for (int k = 0; k < 16; ++k) info[i].icp_final[k] = O.correction[k];
      if (ok) info[i].verified = v;
    }
    return ok;
  }, st, err);
}

// ---- alego_map_align: host ------------------------------------------------------------------------------------------------------------------
int map_align_run(RlCtx* R, LcCtx** lc, const LmCtx& L, const alego_params& P, const int* src, const int* dst, int n, const alego_map_align_opts& o, alego_map_align_result* out,
                  alego_map_align_hyp* hyp_out, hipStream_t st, std::string* err) {
  const char* who = "alego_map_align";
  std::vector<alego_map_align_hyp> hyp((size_t)n * MA_MAX_QUERIES);
  std::memset(hyp.data(), 0, hyp.size() * sizeof(alego_map_align_hyp));
  for (auto& h : hyp) h.src_frame = h.dst_frame = -1;
  for (int i = 0; i < n; ++i) { std::memset(&out[i], 0, sizeof(out[i])); out[i].best = -1; }
  auto finish = [&]() { if (hyp_out && n > 0) std::memcpy(hyp_out, hyp.data(), hyp.size() * sizeof(alego_map_align_hyp)); return 0; };
  if (n == 0) return 0;
  std::vector<int> stat((size_t)R->la_slots * AS_W);
  DevTry t(who, err, "reading the archive");
  if (t.down(stat, arc_stat_of(L, 0), st).wait(st)) return t;
  // the entries: one per (pair, query), in pair order
  std::vector<MaEntry> ent;
  std::vector<RlQuery> qr;
  std::vector<int> pend, first((size_t)n, 0);
  std::vector<char> listed((size_t)R->la_slots, 0);
  for (int i = 0; i < n; ++i) {
    const int ns = std::min(stat[(size_t)src[i] * AS_W + AS_FRAMES], R->la_cap), nd = std::min(stat[(size_t)dst[i] * AS_W + AS_FRAMES], R->la_cap);
    first[i] = (int)ent.size();
    if (stat[(size_t)src[i] * AS_W + AS_DROPPED] > 0 || stat[(size_t)dst[i] * AS_W + AS_DROPPED] > 0) { out[i].status = -1; continue; }
    if (ns == 0 || nd == 0) continue;
    for (int slot : {src[i], dst[i]})
      if (!listed[slot]) {
        listed[slot] = 1;
        const int nf = slot == src[i] ? ns : nd;
        for (int f = std::min(R->la_described[slot], nf); f < nf; ++f) { pend.push_back(slot); pend.push_back(f); }
      }
    const int Q = ma_query_count(ns, o.n_queries);
    out[i].n_queries = Q;
    for (int q = 0; q < Q; ++q) {
      const int f = ma_query_frame(ns, Q, q);
      ent.push_back(MaEntry{src[i], dst[i], f, i});
      RlQuery rq;
      std::memset(&rq, 0, sizeof(rq));
      rq.qrow = src[i] * R->la_cap + f; rq.base = dst[i] * R->la_cap; rq.n = nd; rq.tag = i;
      qr.push_back(rq);
      hyp[(size_t)i * MA_MAX_QUERIES + q].src_frame = f;
    }
  }
  if (int rc = la_describe(R, L, pend, who, st, err)) return rc;
  const int ne = (int)ent.size();
  std::vector<unsigned long long> cand((size_t)ne * ALEGO_RELOC_MAX_CAND + 1);
  if (int rc = rl_search_run(R, R->la_desc, R->la_key, qr.data(), ne, R->la_desc, R->la_key, o.n_cand, cand.data(),
                             [&](const RlQuery* dq, int c, int nmax, uint32_t* bound, int*, hipStream_t s2) {
                               ALEGO_LAUNCH(ma_mask, dim3(std::max(1, (nmax + RL_T - 1) / RL_T), c), dim3(RL_T), 0, s2, dq, (const uint16_t*)R->la_key, bound);
                             }, nullptr, st, err)) return rc;
  if (t.at("descriptors").wait(st)) return t;
  auto hyp_of = [&](int e) -> alego_map_align_hyp& { return hyp[(size_t)ent[e].pair * MA_MAX_QUERIES + (e - first[ent[e].pair])]; };
  std::vector<unsigned long long> ecand((size_t)ne * ALEGO_RELOC_MAX_CAND + 1, RL_CAND_NONE);   // per entry, after the max_dist cut
  std::vector<int> ncand((size_t)ne + 1, 0);
  std::vector<char> tried((size_t)n, 0);
  bool any = false;
  for (int e = 0; e < ne; ++e) {
    int k = 0;
    for (; k < o.n_cand; ++k) {
      const unsigned long long c = cand[(size_t)e * ALEGO_RELOC_MAX_CAND + k];
      if (c == RL_CAND_NONE || (o.max_dist > 0 && rl_cand_dist(c) > o.max_dist)) break;
      ecand[(size_t)e * ALEGO_RELOC_MAX_CAND + k] = c;
    }
    ncand[e] = k;
    if (k > 0) {
      alego_map_align_hyp& H = hyp_of(e);
      H.dst_frame = rl_cand_id(ecand[(size_t)e * ALEGO_RELOC_MAX_CAND]); H.dist = rl_cand_dist(ecand[(size_t)e * ALEGO_RELOC_MAX_CAND]); H.shift = rl_cand_shift(ecand[(size_t)e * ALEGO_RELOC_MAX_CAND]);
      tried[ent[e].pair] = 1; any = true;
    }
  }
  if (!any) return finish();
  // the attempts on every candidate, planned on the device from both archives' tables
  const size_t na = (size_t)ne * ALEGO_RELOC_MAX_CAND;
  if (R->ma_ent.reserve((size_t)ne) != hipSuccess || R->ma_cand.reserve(na) != hipSuccess || R->ma_det.reserve(na) != hipSuccess || R->ma_spose.reserve((size_t)ne * 6) != hipSuccess ||
      R->ma_hyp.reserve((size_t)n * MA_MAX_QUERIES) != hipSuccess || R->ma_nq.reserve((size_t)n) != hipSuccess || R->ma_cons.reserve((size_t)n) != hipSuccess) {
    *err = std::string(who) + ": out of device memory"; return ALEGO_ERR_HIP;
  }
  std::vector<LcDet> plan(na);
  std::vector<float> spose((size_t)ne * 6);
  if (t.at("upload").up(R->ma_ent.p, ent, st).up(R->ma_cand.p, ecand.data(), na, st)) return t;   // (ecand has a spare word past na)
  ALEGO_LAUNCH(ma_plan, dim3(((int)na + 63) / 64), dim3(64), 0, st, L, (const MaEntry*)R->ma_ent.p, (const unsigned long long*)R->ma_cand.p, ne, P.lc_search_num, R->ma_det.p, R->ma_spose.p);
  if (t.at("planning").down(plan, R->ma_det.p, st).down(spose, R->ma_spose.p, st).wait(st)) return t;
  std::vector<int> eslot((size_t)ne);
  for (int e = 0; e < ne; ++e) eslot[e] = ent[e].dst;
  const double fitness_max = o.fitness_max > 0.0 ? o.fitness_max : P.lc_fitness_max;
  if (int rc = loop_rounds(lc, P, R->la_slots, eslot.data(), ne, o.n_cand, loop_archive_gather(L), [&](int e, int v, LcDet* D) {
        if (ncand[e] <= v) return false;
        *D = plan[(size_t)e * ALEGO_RELOC_MAX_CAND + v];
        return D->status == 1;
      }, [&](int e, int v, const LcDet& D, const LcOut& O) {
        alego_map_align_hyp& H = hyp_of(e);
        alego_loop_result r;
        std::memset(&r, 0, sizeof(r));
        const bool ok = loop_result_fill(D, O, fitness_max, &r);
        la_world_correction(r.t_correct, spose.data() + (size_t)e * 6, H.T);
        const unsigned long long c = ecand[(size_t)e * ALEGO_RELOC_MAX_CAND + v];
        H.dst_frame = rl_cand_id(c); H.dist = rl_cand_dist(c); H.shift = rl_cand_shift(c);
        H.tried = v + 1; H.accepted = ok ? 1 : 0;
        H.converged = O.converged; H.iterations = O.iterations; H.n_source = O.n_source; H.n_target = O.n_target; H.fitness = O.fitness;
        for (int k = 0; k < 6; ++k) H.guess6[k] = D.pose_latest[k];
        for (int k = 0; k < 16; ++k) H.icp_final[k] = O.correction[k];
        return ok;
      }, st, err)) return rc;
  // the consensus of every pair's hypotheses
  std::vector<MaHyp> mh((size_t)n * MA_MAX_QUERIES);
  std::memset(mh.data(), 0, mh.size() * sizeof(MaHyp));
  std::vector<int> nq((size_t)n);
  std::vector<MaCons> cons((size_t)n);
  for (int i = 0; i < n; ++i) nq[i] = out[i].n_queries;
  for (int e = 0; e < ne; ++e) {
    const alego_map_align_hyp& H = hyp_of(e);
    MaHyp& M = mh[(size_t)ent[e].pair * MA_MAX_QUERIES + (e - first[ent[e].pair])];
    std::memcpy(M.T, H.T, sizeof(M.T));
    for (int k = 0; k < 3; ++k) M.p[k] = spose[(size_t)e * 6 + k];
    M.accepted = H.accepted; M.fitness = H.fitness;
  }
  const double tol_trans = o.tol_trans > 0.0 ? o.tol_trans : ALEGO_ALIGN_TOL_TRANS, tol_rot = o.tol_rot > 0.0 ? o.tol_rot : ALEGO_ALIGN_TOL_ROT;
  if (t.at("upload").up(R->ma_hyp.p, mh, st).up(R->ma_nq.p, nq, st)) return t;
  ALEGO_LAUNCH(ma_consensus, dim3(n), dim3(64), 0, st, (const MaHyp*)R->ma_hyp.p, (const int*)R->ma_nq.p, tol_trans, tol_rot, R->ma_cons.p);
  if (t.at("the consensus").down(cons, R->ma_cons.p, st).wait(st)) return t;
  const int min_support = o.min_support > 0 ? o.min_support : 2;
  for (int i = 0; i < n; ++i) {
    alego_map_align_result& r = out[i];
    if (r.status < 0 || !tried[i]) continue;
    alego_map_align_hyp* H = &hyp[(size_t)i * MA_MAX_QUERIES];
    for (int q = 0; q < r.n_queries; ++q) { H[q].support = cons[i].support[q]; H[q].inlier = cons[i].inlier[q]; r.n_accepted += H[q].accepted; }
    r.best = cons[i].best;
    r.support = r.best >= 0 ? H[r.best].support : 0;
    r.status = r.best >= 0 && r.support >= min_support ? 2 : 1;
    if (r.best >= 0)
      for (int k = 0; k < 12; ++k) r.T[k] = (double)H[r.best].T[k];
  }
  return finish();
}

extern "C" int alego_map_align_queries(int32_t n_frames, int32_t n_queries, int32_t* frames) {
  if (n_queries <= 0) n_queries = 8;
  if (n_frames < 0 || n_queries > ALEGO_ALIGN_MAX_QUERIES) return ALEGO_ERR_ARG;
  const int Q = ma_query_count(n_frames, n_queries);
  if (Q > 0 && !frames) return ALEGO_ERR_ARG;
  for (int q = 0; q < Q; ++q) frames[q] = ma_query_frame(n_frames, Q, q);
  return Q;
}
extern "C" int alego_map_align_consensus(const float* T16, const float* src_pos3, const double* fitness, const int32_t* accepted, int32_t n, double tol_trans, double tol_rot,
                                         int32_t* support, int32_t* best) {
  if (n < 0 || n > ALEGO_ALIGN_MAX_QUERIES || !best || (n > 0 && (!T16 || !src_pos3 || !fitness || !accepted || !support))) return ALEGO_ERR_ARG;
  *best = ma_consensus_ref(T16, src_pos3, fitness, accepted, n, tol_trans > 0.0 ? tol_trans : ALEGO_ALIGN_TOL_TRANS, tol_rot > 0.0 ? tol_rot : ALEGO_ALIGN_TOL_ROT, support);
  return ALEGO_OK;
}
extern "C" int alego_map_align_poses(const double T12[12], const float* poses6, int32_t n, float* out6) {
  if (!T12 || n < 0 || (n > 0 && (!poses6 || !out6))) return ALEGO_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    float kp[6];   // (out6 may be poses6)
    mg_move_pose6(T12, poses6 + (size_t)i * 6, kp);
    for (int k = 0; k < 6; ++k) out6[(size_t)i * 6 + k] = kp[k];
  }
  return ALEGO_OK;
}

// ---- host twins (plain C++) -----------------------------------------------------------------------------------------------------------
extern "C" int alego_reloc_descriptor(const alego_point* pts, int32_t n, double max_range, double z_offset, uint8_t* desc1200, uint16_t* key20) {
  if (n < 0 || (n > 0 && !pts) || !desc1200 || !key20) return ALEGO_ERR_ARG;
  const float w = rl_ring_width(max_range), zoff = rl_z_offset(z_offset);
  std::memset(desc1200, 0, RL_BYTES);
  for (int i = 0; i < n; ++i) {
    int bin, code;
    if (rl_bin(pts[i].x, pts[i].y, pts[i].z, w, zoff, &bin, &code) && code > desc1200[bin]) desc1200[bin] = (uint8_t)code;
  }
  for (int r = 0; r < RL_NR; ++r) {
    int s = 0;
    for (int c = 0; c < RL_NS; ++c) s += desc1200[c * RL_NR + r];
    key20[r] = (uint16_t)s;
  }
  return ALEGO_OK;
}
extern "C" int alego_reloc_match(const uint8_t* q1200, const uint8_t* m1200, int32_t* dist, int32_t* shift) {
  if (!q1200 || !m1200 || !dist || !shift) return ALEGO_ERR_ARG;
  int best = 0x7fffffff, bs = 0;
  for (int s = 0; s < RL_NS; ++s) {
    int d = 0;
    for (int c = 0; c < RL_NS; ++c) {
      const uint8_t* a = q1200 + ((c + s) % RL_NS) * RL_NR;
      const uint8_t* b = m1200 + c * RL_NR;
      for (int r = 0; r < RL_NR; ++r) d += rl_abs_diff(a[r], b[r]);
    }
    if (d < best) { best = d; bs = s; }
  }
  *dist = best; *shift = bs;
  return ALEGO_OK;
}
// the candidates of the appearance search for frame n - 1 over frames 0 .. n - 2: the brute force over every eligible frame and shift
extern "C" int alego_loop_appearance_candidates(const uint8_t* desc, const float* keyposes6, const double* stamps, int32_t n, double min_time_gap, double max_jump,
                                                int32_t max_dist, int32_t n_cand, int32_t* ids, int32_t* dists, int32_t* shifts) {
  if (n < 0 || n_cand < 1 || n_cand > ALEGO_RELOC_MAX_CAND || (n > 0 && (!desc || !keyposes6 || !stamps)) || !ids || !dists || !shifts) return ALEGO_ERR_ARG;
  if (n < 2) return 0;
  const uint8_t* q = desc + (size_t)(n - 1) * RL_BYTES;
  bool any = false;
  for (int i = 0; i < RL_BYTES; ++i) any = any || q[i] != 0;
  if (!any) return 0;   // no point in range
  const float jump2 = (float)(max_jump * max_jump);
  const float* b = keyposes6 + (size_t)(n - 1) * 6;
  std::vector<unsigned long long> all;   // candidate words
  for (int i = 0; i < n - 1; ++i) {
    if (!(stamps[n - 1] - stamps[i] > min_time_gap)) continue;
    if (max_jump > 0.0) {
      const float* a = keyposes6 + (size_t)i * 6;
      const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
      if (!(((dx * dx) + dy * dy) + dz * dz < jump2)) continue;
    }
    int32_t d, s;
    alego_reloc_match(q, desc + (size_t)i * RL_BYTES, &d, &s);
    all.push_back(rl_cand_pack((uint32_t)d, (uint32_t)i, (uint32_t)s));
  }
  std::sort(all.begin(), all.end());
  int k = 0;
  for (; k < n_cand && k < (int)all.size(); ++k) {
    if (max_dist > 0 && rl_cand_dist(all[k]) > max_dist) break;
    rl_cand_unpack(all.data(), k, ids, dists, shifts);
  }
  return k;
}
