// kernels_occ.hip — the occupancy grid of a slot's key-frame archive by ray casting on gfx950 (alego_occ_*).  The rule is
// occ_math.h's; the host (lm_host.hip) reads the frames' arc_tab rows once and hands over a work list of (frame, chunk of OCC_T selected points).
//
//   occ_cast       one workgroup per work item, two phases.
//                  RAYS: lane i reads point i of the chunk (surf, corner, outlier restricted to `kinds`, as map_gather reads it), transforms it with the
//                  frame's key-pose matrix (built by one lane, kept in LDS), sets the ray up and clips it to the grid: the cells inside are ONE run of
//                  steps [m_in, m_out] of the walk (occ_clip), so no lane ever walks outside the grid and a walk is bounded by n0 + n1 + n2 whatever
//                  the ray's length.  The ray and its run go to LDS.  Every ray of a frame starts in the same cell: the workgroup counts the rays whose
//                  start cell takes a pass (ballot + popcount per wavefront, one LDS add each) and ONE lane adds the sum.
//                  PIECES: the runs are cut into pieces of `piece` steps, numbered by a workgroup scan; lane l takes pieces l, l + OCC_T, ...: it finds
//                  the piece's ray by binary search in the scanned offsets, the walk's state at the piece's first step from the closed form (occ_seek;
//                  the first steps of a ray are walked instead) and adds into hits / passes with u32 atomics.  Every lane walks at most `piece` steps
//                  per round, so a wavefront no longer idles behind its longest ray.  piece <= 0 makes every run one piece: one lane per ray, the
//                  baseline the default was measured against.
//                  The counters go through LDS to six u64 adds per workgroup.  Integer adds: the counts do not depend on the order of arrival.
//   occ_classify   one thread per output cell (or per column with collapse_z): occ_class / occ_class_merge.
//   (clearing is two hipMemsetAsync)
// The static map (alego_occ_mark, alego_map_assemble_static) over the same work items, every frame of a slot:
//   occ_mark       one workgroup per work item: lane i reads point i of the chunk, transforms it as occ_cast does, forms its verdict from its own cell's
//                  counts (occ_static_verdict; the neighbour cells are read only by lanes whose own class is 0) and stores the byte and the
//                  transformed point at the point's position in assembly order (map_offsets' frame offset + index in the frame).  The six
//                  verdict counts go by ballot + popcount per wavefront through LDS to at most six u64 adds per workgroup, the kept count to
//                  one int per item.
//   occ_offsets    one workgroup: exclusive scan of the kept counts, chunk by chunk with a carry (as map_offsets); the total is the cloud's size.
//   occ_emit       one workgroup per work item: the rank of a kept point among the item's kept lanes (block_excl_scan) places it, stably, at
//                  out[off[item] + rank]; out is where gv_filter reads its input.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/alego_mi355x.h"
#include "kf_store.h"
#include "occ.h"
#include "occ_math.h"
#include "prof.h"

#define OCC_SCAN_T 1024  // occ_offsets' workgroup: items scanned per round of its carry
#define OCC_WALK_MIN 8   // a piece that starts within the ray's first steps walks them instead of seeking
// development build -DALEGO_OCC_DRY_RUN (tools/occ_timing.py --dry): the adds of the pieces are left out, the walk and its counter stay - what the traversal
// alone costs ("Measured")
#ifdef ALEGO_OCC_DRY_RUN
#define OCC_ADD(p) ((void)(p))
#else
#define OCC_ADD(p) atomicAdd((p), 1u)
#endif

// rays with more than 2^22 pieces of `piece` steps take longer pieces: the workgroup's piece count stays an int
DEV_INLINE int occ_piece_of(int piece, int cnt) { const int p = (cnt >> 22) + 1; return piece > p ? piece : p; }

__global__ void __launch_bounds__(OCC_T) occ_cast(LmCtx L, OccDev D, int slot, int kinds, const int2* items, int piece) {
  __shared__ float s_m[12];
  __shared__ OccRay s_ray[OCC_T];
  __shared__ long long s_start[OCC_T];
  __shared__ int s_cnt[OCC_T], s_off[OCC_T], s_w[OCC_T / 64];
  __shared__ unsigned long long s_stat[ALEGO_OCC_STATS];
  __shared__ int s_first;
  const int tid = threadIdx.x;
  const int2 it = items[blockIdx.x];
  const KfArcFrame A = kf_arc_frame(L, slot, it.x);
  const int n = kf_sel_count(A, kinds);
  if (tid == 0) {
    float m[3][4];
    keypose_matrix(A.pose, m);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) s_m[r * 4 + c] = m[r][c];
    s_first = 0;
  }
  if (tid < ALEGO_OCC_STATS) s_stat[tid] = 0;
  __syncthreads();
  const OccGrid& G = D.G;
  // ---- rays
  const int i = it.y * OCC_T + tid;
  int code = 1, truncated = 0, cnt = 0;
  long long start = 0;
  bool first = false;
  unsigned long long upd = 0;
  if (i < n) {
    float m[3][4];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[r][c] = s_m[r * 4 + c];
    const float4 p = kf_transform(m, A.pts[kf_arc_index(A.nc, A.ns, kinds, i)]);
    const float o[3] = {m[0][3], m[1][3], m[2][3]}, e[3] = {p.x, p.y, p.z};
    OccRay R;
    code = occ_ray_setup(G, o, e, &R);
    truncated = R.truncated;
    int64_t m_in, m_out;
    if (code == 0 && occ_clip(G, R, &m_in, &m_out)) {
      if (m_in == 0) {   // the start cell lies inside: the workgroup counts it, unless it is the ray's only cell
        if (R.total == 0) {
          if (occ_inside(G, R.c0)) { atomicAdd((R.truncated ? D.passes : D.hits) + occ_index(G, R.c0), 1u); ++upd; }
        } else {
          first = true;
        }
        m_in = 1;
      }
      if (m_in <= m_out) { start = m_in; cnt = (int)(m_out - m_in + 1); }
      s_ray[tid] = R;
    }
  }
  const int pl = occ_piece_of(piece > 0 ? piece : 0x7fffffff, cnt);
  const int np = (int)(((long long)cnt + pl - 1) / pl);
  int tot;
  const int ex = block_excl_scan<OCC_T / 64>(np, s_w, &tot);
  s_off[tid] = ex; s_start[tid] = start; s_cnt[tid] = cnt;
  {
    const unsigned long long b_ray = __ballot(code != 1), b_short = __ballot(code == ALEGO_OCC_SKIP_SHORT), b_trunc = __ballot(truncated != 0),
                             b_cull = __ballot(code == ALEGO_OCC_SKIP_CULLED), b_bad = __ballot(code == ALEGO_OCC_SKIP_BAD), b_first = __ballot(first);
    if ((tid & 63) == 0) {
      if (b_ray) atomicAdd(&s_stat[ALEGO_OCC_RAYS], (unsigned long long)__popcll(b_ray));
      if (b_short) atomicAdd(&s_stat[ALEGO_OCC_SHORT], (unsigned long long)__popcll(b_short));
      if (b_trunc) atomicAdd(&s_stat[ALEGO_OCC_TRUNCATED], (unsigned long long)__popcll(b_trunc));
      if (b_cull) atomicAdd(&s_stat[ALEGO_OCC_CULLED], (unsigned long long)__popcll(b_cull));
      if (b_bad) atomicAdd(&s_stat[ALEGO_OCC_BAD], (unsigned long long)__popcll(b_bad));
      if (b_first) atomicAdd(&s_first, __popcll(b_first));
    }
  }
  __syncthreads();
  if (tid == 0 && s_first > 0) {   // the frame's start cell: the same expression as occ_ray_setup's, and inside the grid since a ray counted it
    int32_t c0[3];
    for (int k = 0; k < 3; ++k) c0[k] = (int32_t)floor(occ_coord(G, k, (double)s_m[k * 4 + 3]));
    if (occ_inside(G, c0)) { atomicAdd(D.passes + occ_index(G, c0), (unsigned)s_first); upd += (unsigned long long)s_first; }
  }
  // ---- pieces
  for (int p = tid; p < tot; p += OCC_T) {
    int lo = 0, hi = OCC_T - 1;   // the last ray whose offset is <= p (a ray without pieces shares its offset with the next one)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const OccRay R = s_ray[lo];
    const int rc = s_cnt[lo], rp = occ_piece_of(piece > 0 ? piece : 0x7fffffff, rc);
    const long long q = p - s_off[lo];
    const long long a = s_start[lo] + q * rp;
    const int len = (int)((long long)rc - q * rp < rp ? (long long)rc - q * rp : rp);
    OccWalk W;
    if (a <= OCC_WALK_MIN) {
      occ_walk_begin(G, R, &W);
      for (int s = 0; s < (int)a; ++s) occ_step(G, R, &W);
    } else {
      int64_t j[3];
      occ_seek(G, R, a, j);
      occ_walk_at(G, R, j, &W);
    }
    for (int s = 0; s < len; ++s) {
      const long long mi = a + s;
      if (occ_inside(G, W.c)) {   // (always, by occ_clip: the test keeps a fault in it from becoming a write outside the arrays)
        OCC_ADD(((mi == R.total && !R.truncated) ? D.hits : D.passes) + occ_index(G, W.c));
        ++upd;
      }
      if (mi < R.total) occ_step(G, R, &W);
    }
  }
  if (upd) atomicAdd(&s_stat[ALEGO_OCC_UPDATES], upd);
  __syncthreads();
  if (tid < ALEGO_OCC_STATS && s_stat[tid]) atomicAdd(D.stats + tid, s_stat[tid]);
}

__global__ void __launch_bounds__(OCC_T) occ_classify(OccDev D, alego_occ_rule rule, int collapse_z, int8_t* out) {
  const size_t layer = (size_t)D.G.n[0] * D.G.n[1], cells = layer * D.G.n[2];
  const size_t n_out = collapse_z ? layer : cells;
  for (size_t i = (size_t)blockIdx.x * OCC_T + threadIdx.x; i < n_out; i += (size_t)gridDim.x * OCC_T) {
    if (!collapse_z) { out[i] = occ_class(rule, D.hits[i], D.passes[i]); continue; }
    int8_t col = -1;
    for (int z = 0; z < D.G.n[2]; ++z) col = occ_class_merge(col, occ_class(rule, D.hits[z * layer + i], D.passes[z * layer + i]));
    out[i] = col;
  }
}

// ---- the static map
__global__ void __launch_bounds__(OCC_T) occ_mark(LmCtx L, OccDev D, OccStatic S, alego_static_rule rule, int slot, int kinds) {
  __shared__ float s_m[12];
  __shared__ unsigned s_stat[ALEGO_STATIC_VERDICTS];
  const int tid = threadIdx.x;
  const int2 it = S.items[blockIdx.x];
  const KfArcFrame A = kf_arc_frame(L, slot, it.x);
  const int n = kf_sel_count(A, kinds);
  if (tid == 0) {
    float m[3][4];
    keypose_matrix(A.pose, m);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) s_m[r * 4 + c] = m[r][c];
  }
  if (tid < ALEGO_STATIC_VERDICTS) s_stat[tid] = 0;
  __syncthreads();
  const int i = it.y * OCC_T + tid;
  const long long pos = (long long)S.frame_off[it.x] + i;
  int v = -1;
  if (i < n && pos >= 0 && pos < S.n_pts) {   // (pos < n_pts always, by map_offsets: the test keeps a fault in it from becoming a write outside the arrays)
    float m[3][4];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[r][c] = s_m[r * 4 + c];
    const float4 raw = A.pts[kf_arc_index(A.nc, A.ns, kinds, i)];
    const float4 p = kf_transform(m, raw);
    const float e[3] = {p.x, p.y, p.z};
    v = occ_static_verdict(D.G, rule, D.hits, D.passes, e, raw.z);
    S.verdict[pos] = (uint8_t)v;
    S.pts[pos] = p;
  }
#pragma unroll
  for (int k = 0; k < ALEGO_STATIC_VERDICTS; ++k) {
    const unsigned long long b = __ballot(v == k);
    if ((tid & 63) == 0 && b) atomicAdd(&s_stat[k], (unsigned)__popcll(b));
  }
  __syncthreads();
  if (tid < ALEGO_STATIC_VERDICTS && s_stat[tid]) atomicAdd(S.stats + tid, (unsigned long long)s_stat[tid]);
  if (tid == 0) {
    unsigned kept = 0;
    for (int k = 0; k < ALEGO_STATIC_VERDICTS; ++k) if (k != ALEGO_STATIC_REMOVED) kept += s_stat[k];
    S.kept[blockIdx.x] = (int)kept;
  }
}

// one workgroup: off[i] = kept points of the items [0, i), off[n_items] = *n = the total
__global__ void __launch_bounds__(OCC_SCAN_T) occ_offsets(const int* kept, int n_items, int* off, int* n) {
  __shared__ int s_w[OCC_SCAN_T / 64];
  int carry = 0;
  for (int i0 = 0; i0 < n_items; i0 += OCC_SCAN_T) {
    const int i = i0 + threadIdx.x;
    const int v = i < n_items ? kept[i] : 0;
    int tot;
    const int ex = block_excl_scan<OCC_SCAN_T / 64>(v, s_w, &tot);
    if (i < n_items) off[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) { off[n_items] = carry; *n = carry; }
}

__global__ void __launch_bounds__(OCC_T) occ_emit(OccStatic S, int kinds, float4* out, int out_cap) {
  __shared__ int s_w[OCC_T / 64];
  const int2 it = S.items[blockIdx.x];
  const int f0 = S.frame_off[it.x], n = S.frame_off[it.x + 1] - f0;   // the frame's selected points, as occ_mark counted them
  const int i = it.y * OCC_T + threadIdx.x;
  const long long pos = (long long)f0 + i;
  const bool keep = i < n && pos >= 0 && pos < S.n_pts && S.verdict[pos] != ALEGO_STATIC_REMOVED;
  int tot;
  const int rank = block_excl_scan<OCC_T / 64>(keep ? 1 : 0, s_w, &tot);
  const long long o = (long long)S.off[blockIdx.x] + rank;
  if (keep && o >= 0 && o < out_cap) {
    float4 p = S.pts[pos];
    if (kinds & 8) p.w = (float)it.x;
    out[o] = p;
  }
}

void launch_occ_mark(const LmCtx& L, const OccDev& D, const OccStatic& S, const alego_static_rule& rule, int slot, int kinds, hipStream_t st) {
  (void)hipMemsetAsync(S.stats, 0, ALEGO_STATIC_VERDICTS * sizeof(unsigned long long), st);
  if (S.n_items > 0) ALEGO_LAUNCH(occ_mark, dim3(S.n_items), dim3(OCC_T), 0, st, L, D, S, rule, slot, kinds);
}
void launch_occ_emit(const OccStatic& S, int kinds, float4* out, int out_cap, int* n_dev, hipStream_t st) {
  ALEGO_LAUNCH(occ_offsets, dim3(1), dim3(OCC_SCAN_T), 0, st, S.kept, S.n_items, S.off, n_dev);
  if (S.n_items > 0) ALEGO_LAUNCH(occ_emit, dim3(S.n_items), dim3(OCC_T), 0, st, S, kinds, out, out_cap);
}

void launch_occ_cast(const LmCtx& L, const OccDev& D, int slot, int kinds, const int2* items, int n_items, int piece, hipStream_t st) {
  if (n_items > 0) ALEGO_LAUNCH(occ_cast, dim3(n_items), dim3(OCC_T), 0, st, L, D, slot, kinds, items, piece);
}
void launch_occ_classify(const OccDev& D, alego_occ_rule rule, int collapse_z, int8_t* out, hipStream_t st) {
  const size_t n_out = collapse_z ? (size_t)D.G.n[0] * D.G.n[1] : occ_cells(D.G);
  const int nb = (int)std::min<size_t>((n_out + OCC_T - 1) / OCC_T, 65536);
  ALEGO_LAUNCH(occ_classify, dim3(nb), dim3(OCC_T), 0, st, D, rule, collapse_z, out);
}
void launch_occ_clear(const OccDev& D, hipStream_t st) {
  (void)hipMemsetAsync(D.hits, 0, occ_cells(D.G) * sizeof(uint32_t), st);
  (void)hipMemsetAsync(D.passes, 0, occ_cells(D.G) * sizeof(uint32_t), st);
}
