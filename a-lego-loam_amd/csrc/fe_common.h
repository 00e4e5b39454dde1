// fe_common.h — what the feature-extraction kernels of kernels_fe.hip and kernels_fe2.hip share on the device: the body of fe_curv (curvature +
// occlusion marks of a chunk of the segmented cloud, src/laserOdometry.cpp:122-159), the ring-ascending concatenation of per-ring lists into a
// feature cloud with its bounding boxes (:199-205,:245,:293), and the bucket tables that order the runs of a ring's VoxelGrid.  The rules
// themselves are fe_rules.h (host-readable).
#ifndef ALEGO_FE_COMMON_H_
#define ALEGO_FE_COMMON_H_
#include "dev_common.h"
#include "fe_rules.h"

#define FE_HALO 6

DEV_INLINE int fe_sector_start(const alego_params& P, int S, int E, int j) { return fe_sector_start(P.sector_formula, P.n_sectors, S, E, j); }
DEV_INLINE void fe_sector(const alego_params& P, int S, int E, int j, int& sp, int& ep) { fe_sector(P.sector_formula, P.n_sectors, S, E, j, sp, ep); }
DEV_INLINE unsigned fe_occl_marks(const alego_params& P, float r_prev, float r0, float r1, int c0, int c1) {
  return fe_occl_marks(P.occl_f32, P.occl_depth, P.occl_col_diff, P.parallel_ratio, r_prev, r0, r1, c0, c1);
}
template <bool FLAT>
DEV_INLINE void fe_pick_label(const alego_params& P, int picked, int nmax, int& lab, bool& spread, bool& more) {
  fe_pick_label<FLAT>(P.n_sharp, P.n_less_sharp, P.n_flat, picked, nmax, lab, spread, more);
}

// points [t0, t0 + CW) of slot `slot` by a workgroup of BLOCK threads; s_r / s_c / s_f hold CW + 2 FE_HALO entries.
//   cd[i]       fe_curv_sum
//   fe_flag[i]  fe_flag_of(fe_point_picked, ground, curvature thresholds, label 0, jump to the next point)
//   picked0[i]  bit 0 alone, for the single-scan entry points / tests
// The caller synchronises before s_r / s_c / s_f are reused.
template <int BLOCK, int CW>
DEV_INLINE void fe_curv_chunk(const DevCtx& d, int slot, int M, int t0, float* s_r, int* s_c, uint8_t* s_f) {
  const size_t base = (size_t)slot * d.N;
  const float* rng = d.seg_range + base;
  const int* colv = d.seg_col + base;
  const alego_params& P = d.P;
#pragma unroll 4
  for (int j = threadIdx.x; j < CW + 2 * FE_HALO; j += BLOCK) {
    const int i = t0 - FE_HALO + j;
    const bool in = i >= 0 && i < M;
    s_r[j] = in ? rng[i] : 0.f;
    s_c[j] = in ? colv[i] : 0;
  }
  __syncthreads();
  for (int j = threadIdx.x + 1; j < CW + 2 * FE_HALO - 1; j += BLOCK) {
    const int i = t0 - FE_HALO + j;
    s_f[j] = fe_has_taps(i, M) ? (uint8_t)fe_occl_marks(P, s_r[j - 1], s_r[j], s_r[j + 1], s_c[j], s_c[j + 1]) : (uint8_t)0;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < CW / BLOCK; ++u) {
    const int i = t0 + u * BLOCK + threadIdx.x;
    if (i >= M) break;
    const int j = u * BLOCK + threadIdx.x + FE_HALO;
    const float cdv = fe_has_taps(i, M) ? fe_curv_sum(s_r + j) : 0.f;
    const bool pk = fe_point_picked(s_f + j);
    const double curv = fe_curvature(cdv);
    d.cd[base + i] = cdv;
    d.fe_flag[base + i] = fe_flag_of(pk, d.seg_ground[base + i] != 0, fe_curv_edge(curv, P.edge_thres), fe_curv_surf(curv, P.surf_thres), 0,
                                     i + 1 < M && fe_col_jump(s_c[j], s_c[j + 1], P.suppress_col_diff));
    if (d.n_launch == 1) d.picked0[base + i] = pk ? 1 : 0;
  }
}

// ---- ring-ascending concatenation ----
// off[r] = first output point of ring r, off[64] = the total (rings beyond NS hold the total).  The exclusive scan of one count per ring, by the
// workgroup's first wavefront (lane = ring); the caller's barrier follows.
DEV_INLINE void fe_ring_offsets(int c, int* off) {
  const int incl = wave_incl_scan(c);
  off[threadIdx.x] = incl - c;
  if (threadIdx.x == 63) off[64] = incl;
}
DEV_INLINE int fe_ring_of(const int* off, int NS, int i) {   // largest r with off[r] <= i (never a ring beyond NS for i < total)
  int lo = 0, hi = NS - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= i) lo = mid; else hi = mid - 1; }
  return lo;
}
// One cloud: output point off[r] + j = src(r, j, off[r] + j), which also stores whatever else belongs to the point.  boff = nullptr: point by
// point.  Otherwise boff[r] = first box of ring r (boxes never straddle rings) and the cloud is walked box by box — LO_CH consecutive threads
// = the up to LO_CH points of one ring's box — and bx gets every box's corners, first point and length, for the next scan's LaserOdometry.
template <int BLOCK, class Src>
DEV_INLINE void fe_concat_cloud(int NS, const int* off, const int* boff, float4* dst, float4* bx, Src src) {
  const int tid = threadIdx.x;
  const bool boxes = boff != nullptr;
  const int nwork = boxes ? boff[64] * LO_CH : off[64];
  for (int i0 = 0; i0 < nwork; i0 += BLOCK) {
    int i = i0 + tid, r = 0, j = 0, bxi = 0;
    bool v = i < nwork;
    if (boxes) {
      bxi = min(i / LO_CH, boff[64] - 1);
      r = fe_ring_of(boff, NS, bxi); j = (bxi - boff[r]) * LO_CH + (tid % LO_CH);
      v = v && j < off[r + 1] - off[r];
      i = off[r] + j;
    } else if (v) { r = fe_ring_of(off, NS, i); j = i - off[r]; }
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v) { p = src(r, j, i); dst[i] = p; }
    if (boxes) {
      float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
      if (v) { mn[0] = mx[0] = p.x; mn[1] = mx[1] = p.y; mn[2] = mx[2] = p.z; }
#pragma unroll
      for (int a = 0; a < 3; ++a)
        bfly_minmax_f32<LO_CH>(mn[a], mx[a]);
      if ((tid % LO_CH) == 0 && v) {   // (thread 0 of a box holds its first point: every box has one)
        bx[2 * bxi] = make_float4(mn[0], mn[1], mn[2], __int_as_float(i));
        bx[2 * bxi + 1] = make_float4(mx[0], mx[1], mx[2], __int_as_float(min(LO_CH, off[r + 1] - i)));
      }
    }
  }
}
// The three pick clouds of a stream from the per-ring index lists (sharp, less_sharp, flat: :199-205,:245), their index lists and counts, the
// less_sharp ring offsets and boxes; with_plabel: cloud_label_ from the lists as well (2 sharp, 1 less sharp, -1 flat, 0 otherwise), for a path
// whose pick keeps no label per point.  s_off: [0..2] first pick of every ring in the three clouds, [3] first less_sharp box.  One workgroup of
// BLOCK >= 65 threads; ends with the offsets still readable.
template <int BLOCK>
DEV_INLINE void fe_concat_picks(const DevCtx& d, int slot, size_t fb, int (*s_off)[65], bool with_plabel) {
  const int tid = threadIdx.x, NS = d.NS;
  const size_t base = (size_t)slot * d.N;
  const int* allc = st_cnt_of(d, slot, 0);
  const float4* seg = d.seg_lo + base;
  if (tid < 64) {
    const int r = tid;
    int c[4];
    c[0] = r < NS ? allc[r * ST_W + F_SHARP] : 0; c[1] = r < NS ? allc[r * ST_W + F_LSHARP] : 0; c[2] = r < NS ? allc[r * ST_W + F_FLAT] : 0;
    c[3] = (c[1] + LO_CH - 1) / LO_CH;
#pragma unroll
    for (int k = 0; k < 4; ++k) fe_ring_offsets(c[k], s_off[k]);
  }
  __syncthreads();
  if (tid <= NS) {
    ring_off_of(d, fb, RO_LSHARP)[tid] = tid < NS ? s_off[1][tid] : s_off[1][64];
    ring_boff_of(d, fb, RO_LSHARP)[tid] = tid < NS ? s_off[3][tid] : s_off[3][64];
  }
  if (tid < 3) feat_cnt_of(d, fb)[tid] = s_off[tid][64];
  const int stoff[3] = {st_part(d, F_SHARP), st_part(d, F_LSHARP), st_part(d, F_FLAT)};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int* dsti = feat_idx_of(d, k, fb);
    const int so = stoff[k];
    fe_concat_cloud<BLOCK>(NS, s_off[k], k == F_LSHARP ? s_off[3] : nullptr, feat_of(d, k, fb), lo_box_of(d, lo_row(fb, box_set_of(F_LSHARP))),
                           [&](int r, int j, int i) -> float4 { const int idx = st_idx_of(d, slot, r)[so + j]; dsti[i] = idx; return seg[idx]; });
  }
  if (with_plabel) {
    const int M = scal_of(d, slot)[SC_M];
    for (int k = tid; k < M; k += BLOCK) d.plabel[base + k] = 0;
    __syncthreads();
    for (int pass = 0; pass < 3; ++pass) {   // less sharp first: a sharp pick is on both lists
      const int k = pass == 0 ? 1 : (pass == 1 ? 0 : 2), lab = pass == 0 ? 1 : (pass == 1 ? 2 : -1);
      for (int i = tid; i < s_off[k][64]; i += BLOCK) {
        const int r = fe_ring_of(s_off[k], NS, i);
        d.plabel[base + st_idx_of(d, slot, r)[stoff[k] + i - s_off[k][r]]] = lab;
      }
      __syncthreads();
    }
  }
}

// ---- ordering the runs of a ring's VoxelGrid by voxel id: <= NB buckets monotone in the id ----
// Voxel ids are bounded by the grid size T: bucket = id >> shift, clamped (ids wrap when T passes 2^32).
struct FeBuckets { int shift, nb; };
DEV_INLINE FeBuckets fe_buckets(unsigned long long T, int NB) {
  T = max(T, 1ull);
  FeBuckets b;
  b.shift = 0;
  while (((T - 1) >> b.shift) >= (unsigned)NB) ++b.shift;
  b.nb = (int)((T - 1) >> b.shift) + 1;
  return b;
}
DEV_INLINE int fe_bucket_of(const FeBuckets& b, uint32_t vid) { return min((int)(vid >> b.shift), b.nb - 1); }
// the runs are counted into s_boff[bucket + 1] between these two (LDS atomics; the caller's barriers around them)
template <int BLOCK>
DEV_INLINE void fe_buckets_clear(int nb, int* s_boff) { for (int b = threadIdx.x; b <= nb; b += BLOCK) s_boff[b] = 0; }
// inclusive scan of s_boff[1..nb] (NB / BLOCK consecutive entries per thread) -> bucket b = [s_boff[b], s_boff[b + 1]); s_bcur[b] starts at
// s_boff[b] (written one slot up, read one down).  One barrier inside; the caller's barrier follows.  s_scan: BLOCK / 64 ints.
template <int BLOCK, int NB>
DEV_INLINE void fe_buckets_scan(int nb, int* s_boff, int* s_bcur, int* s_scan) {
  const int tid = threadIdx.x;
  constexpr int PER = NB / BLOCK;
  int v[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) { const int b = tid * PER + k; v[k] = b < nb ? s_boff[b + 1] : 0; sum += v[k]; }
  const int incl = wave_incl_scan(sum);
  if ((tid & 63) == 63) s_scan[tid >> 6] = incl;
  __syncthreads();
  int run = incl - sum;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; ++w) if (w < (tid >> 6)) run += s_scan[w];
#pragma unroll
  for (int k = 0; k < PER; ++k) { const int b = tid * PER + k; run += v[k]; if (b < nb) { s_boff[b + 1] = run; s_bcur[b + 1] = run; } }
  if (tid == 0) s_bcur[0] = 0;
}
#endif
