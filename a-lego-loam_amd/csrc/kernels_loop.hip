// kernels_loop.hip — performLoopClosure + detectLoopClosure (src/laserMapping.cpp:652-824) for many slots at once, read straight from
// the device key-frame archive (alego_map_enable).  The host keeps the pose graph; this is the per-point work of one attempt per slot.
//
//   lc_detect    one workgroup per listed slot: the (d², id) arg-min over the archived key poses within lc_search_radius of the
//                slot's t_map2laser_ whose stamp is more than lc_min_time_gap older than the newest frame's (:771-790), the history
//                window closest ± lc_search_num (< latest, >= 0) and the sizes of the source and of the raw sub-map
//   lc_gather    one workgroup per (attempt, frame): the newest frame (source) under det.pose_latest — its archived key pose for
//                alego_loop_search, the guess for the appearance search (kernels_reloc.hip) — and the history frames under their archived
//                key poses (keypose_matrix / kf_transform, as map_gather), surf, corner, outlier per frame (:794-807) through kf_store.h's view
//   (voxel.h)    VoxelGrid(lc_leaf) of every slot's raw sub-map: one job per slot of the one-workgroup kernels (bit-exact)
//   lc_grid      one workgroup per slot: stable counting sort of the filtered target into a uniform grid of power-of-two cells,
//                with every cell's actual f32 bounding box
//   lc_icp       one workgroup per slot runs the whole alignment: per iteration the previous transformation_ applied in f32, the
//                exact 1-NN of every source point through the grid (lc_nn), the 17 f64 sums (each thread sums its own points in
//                index order, then a fixed butterfly / wave order), Horn's step and the convergence test (icp_math.h) on one thread;
//                then getFitnessScore().  No workgroup waits for another; results do not depend on which slots share a launch.
// The host side offers the attempts to the other callers (loop_ctx.h): loop_attempts with a gather of the caller's (loop_archive_gather: lc_gather),
// loop_rounds, the verification rounds of relocalisation and of the appearance search, and loop_result_fill, the alego_loop_result of a verdict.
//
// Exactness of lc_nn.  The answer must be the brute force's: the smallest nn_d2, ties to the lowest target index, for
// queries anywhere.  Candidates are compared as the (d², index) pair (nn_better), so the visiting order does not matter.  A cell is skipped
// only when nn_beyond holds for the bound to its actual f32 box; shells of cells are visited outward from the query's (clamped) cell and the
// search stops when nn_beyond holds for the half-spaces beyond the visited block.  The bounds, the cells and their argument: nn_rules.h.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "dev_copy.h"
#include "dev_mem.h"
#include "icp_math.h"
#include "kf_store.h"
#include "loop_ctx.h"
#include "nn_rules.h"
#include "prof.h"
#include "voxel.h"

#define LC_DT 256     // lc_detect / lc_gather / lc_grid
#define LC_IT 512     // lc_icp

struct LcGrid { double mn[3], slack[3], h, inv_h; int g[3], ncell; };

// ---- detection ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LC_DT) lc_detect(LmCtx L, const int* list, alego_params P, LcDet* det) {
  __shared__ unsigned long long s_min[LC_DT / 64];
  const int b = blockIdx.x, slot = list[b];
  const int* st = arc_stat_of(L, slot);
  const int nf = st[AS_FRAMES], dropped = st[AS_DROPPED];
  LcDet D;
  memset(&D, 0, sizeof(D));
  D.latest = nf - 1; D.closest = -1; D.jlo = 0; D.jhi = -1;
  if (dropped > 0 || nf == 0) {   // frames missing: the newest key frame is not in the archive; none yet: performLoopClosure returns (:654)
    D.status = dropped > 0 ? -1 : 0;
    if (threadIdx.x == 0) det[b] = D;
    return;
  }
  const double* ld = L.ld + (size_t)slot * LD_COUNT;
  const float cx = (float)ld[LD_T_M2L + 0], cy = (float)ld[LD_T_M2L + 1], cz = (float)ld[LD_T_M2L + 2];
  const float r2 = nn_r2(P.lc_search_radius);
  const size_t fb = arc_row(L, slot, 0);
  const double t_last = L.arc_stamp[fb + nf - 1];
  nn_key_t best = NN_NONE;
  for (int i = threadIdx.x; i < nf; i += LC_DT) {
    const float* kp = arc_pose_of(L, slot, i);
    const float r = nn_d2(kp[0], kp[1], kp[2], cx, cy, cz);
    // radiusSearch (:778) + the first candidate in (d², id) order that is old enough (:781-788)
    if (nn_in_radius(r, r2) && t_last - L.arc_stamp[fb + i] > P.lc_min_time_gap) best = min(best, nn_key(r, (uint32_t)i));
  }
  best = block_min_u64<LC_DT / 64>(best, s_min);
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 6; ++k) D.pose_latest[k] = arc_pose_of(L, slot, nf - 1)[k];
  if (best != NN_NONE) {
    D.status = 1;
    D.closest = nn_key_index(best);
    for (int k = 0; k < 6; ++k) D.pose_closest[k] = arc_pose_of(L, slot, D.closest)[k];
    lc_window(D.closest, P.lc_search_num, D.latest - 1, &D.jlo, &D.jhi);   // :798-803: j < 0 || j >= latest_history_frame_id_ are skipped
  }
  lc_det_sizes(L, slot, nf - 1, &D);   // (no candidate: the window is empty)
  det[b] = D;
}

// ---- sub-map --------------------------------------------------------------------------------------------------------------------
// grid (1 + frames, jobs): x = 0 the source — archived frame det.latest of the source's slot (lc_src_slot: the job's own unless the attempt
// names another) under det.pose_latest; x = 1 + k the history frame jlo + k of the job's slot under its key pose
__global__ void __launch_bounds__(LC_DT) lc_gather(LmCtx L, const LcJob* jobs, const LcDet* det, float4* src, float4* raw) {
  const LcJob J = jobs[blockIdx.y];
  const LcDet& D = det[J.li];
  const bool source = blockIdx.x == 0;
  const int f = source ? D.latest : D.jlo + (int)blockIdx.x - 1;
  if (!source && f > D.jhi) return;
  float4* out = source ? src + J.src_off : lc_frame_out(raw, J, D, f, [&](int j) { return arc_tab_points(arc_tab_of(L, J.slot, j)); });
  const KfArcFrame A = kf_arc_frame(L, source ? lc_src_slot(D, J.slot) : J.slot, f);
  float m[3][4];
  keypose_matrix(source ? D.pose_latest : A.pose, m);
  kf_clouds_write<LC_DT>(kf_clouds(A), m, out);
}

// ---- uniform grid ---------------------------------------------------------------------------------------------------------------
DEV_INLINE int lc_axis(const LcGrid& G, int a, float x) { return nn_lc_axis(x, G.mn[a], G.inv_h, G.g[a]); }
DEV_INLINE int lc_cell(const LcGrid& G, const float4& p) { return nn_lc_index(lc_axis(G, 0, p.x), lc_axis(G, 1, p.y), lc_axis(G, 2, p.z), G.g[0], G.g[1]); }

// the grid of n points (one workgroup of LC_DT threads): cells of 2^k (the smallest k with at most max(1, min(n / 8, cell_cap - 1)) cells),
// cstart[ncell + 1] = first sorted position of every cell, cbox[2 c], [2 c + 1] = min / max xyz of the cell's points, spts = the points in
// cell order (index order inside a cell), w = target index
DEV_INLINE void lc_grid_build(const float4* P, int n, int cell_cap, LcGrid* geo, int* cstart, int* ccur, float4* cbox, float4* spts) {
  __shared__ float s_r[6][LC_DT / 64];
  __shared__ LcGrid s_g;
  __shared__ int s_cell[LC_DT];
  __shared__ int s_w[17];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = threadIdx.x; i < n; i += LC_DT) {
    const float4 p = P[i];
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    bfly_minmax_f32(mn[a], mx[a]);
  if (lane_id() == 0) for (int a = 0; a < 3; ++a) { s_r[a][threadIdx.x >> 6] = mn[a]; s_r[3 + a][threadIdx.x >> 6] = mx[a]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    LcGrid G;
    double e[3], emax = 0.0;
    for (int a = 0; a < 3; ++a) {
      float lo = s_r[a][0], hi = s_r[3 + a][0];
      for (int w = 1; w < LC_DT / 64; ++w) { lo = fminf(lo, s_r[a][w]); hi = fmaxf(hi, s_r[3 + a][w]); }
      if (n == 0) { lo = 0.f; hi = 0.f; }
      G.mn[a] = lo; e[a] = (double)hi - (double)lo; emax = fmax(emax, e[a]);
    }
    const int k = nn_lc_cell_exp(e, emax, (double)max(1, min(n / 8, cell_cap - 1)));
    G.h = ldexp(1.0, k); G.inv_h = ldexp(1.0, -k);
    G.ncell = 1;
    for (int a = 0; a < 3; ++a) {
      G.g[a] = (int)(floor(e[a] * G.inv_h) + 1.0);
      G.ncell *= G.g[a];
      G.slack[a] = nn_face_slack(G.mn[a], e[a], G.h);
    }
    if (n == 0) G.ncell = 0;
    s_g = G;
    *geo = G;
  }
  __syncthreads();
  const LcGrid G = s_g;
  for (int c = threadIdx.x; c <= G.ncell; c += LC_DT) cstart[c] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += LC_DT) atomicAdd(&cstart[lc_cell(G, P[i])], 1);
  __syncthreads();
  int carry = 0;   // exclusive scan of the counts (in place), chunk by chunk
  for (int c0 = 0; c0 < G.ncell; c0 += LC_DT) {
    const int c = c0 + threadIdx.x;
    const int v = c < G.ncell ? cstart[c] : 0;
    int tot;
    const int ex = carry + block_excl_scan<LC_DT / 64>(v, s_w, &tot);
    if (c < G.ncell) { cstart[c] = ex; ccur[c] = ex; }
    carry += tot;
  }
  if (threadIdx.x == 0) cstart[G.ncell] = n;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += LC_DT) {   // stable scatter: rank among the earlier points of the same cell in this round
    const int i = i0 + threadIdx.x;
    const int c = i < n ? lc_cell(G, P[i]) : -1;
    s_cell[threadIdx.x] = c;
    __syncthreads();
    int rank = 0, later = 0;
    const int m = min(LC_DT, n - i0);
    for (int j = 0; j < m; ++j) { const int cj = s_cell[j]; if (cj == c) { if (j < (int)threadIdx.x) ++rank; else if (j > (int)threadIdx.x) ++later; } }
    if (i < n) {
      float4 p = P[i];
      p.w = __int_as_float(i);
      spts[ccur[c] + rank] = p;
    }
    __syncthreads();
    if (i < n && later == 0) ccur[c] += rank + 1;
    __syncthreads();
  }
  for (int c = threadIdx.x; c < G.ncell; c += LC_DT) {
    float4 lo = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.f), hi = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.f);
    bool any = false;
    for (int j = cstart[c]; j < cstart[c + 1]; ++j) {
      const float4 p = spts[j];
      any = true;
      lo.x = fminf(lo.x, p.x); lo.y = fminf(lo.y, p.y); lo.z = fminf(lo.z, p.z);
      hi.x = fmaxf(hi.x, p.x); hi.y = fmaxf(hi.y, p.y); hi.z = fmaxf(hi.z, p.z);
    }
    if (!any) { lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f); hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f); }
    cbox[2 * (size_t)c] = lo; cbox[2 * (size_t)c + 1] = hi;
  }
}

__global__ void __launch_bounds__(LC_DT) lc_grid(const LcJob* jobs, const int* n_tgt, const float4* tgt, LcGrid* geo, int* cstart, int* ccur, float4* cbox, float4* spts) {
  const LcJob J = jobs[blockIdx.x];
  lc_grid_build(tgt + J.raw_off, n_tgt[blockIdx.x], J.cell_cap, geo + blockIdx.x, cstart + J.cell_off, ccur + J.cell_off, cbox + 2 * (size_t)J.cell_off, spts + J.raw_off);
}

// ---- exact 1-NN -----------------------------------------------------------------------------------------------------------------
DEV_INLINE double lc_box_d2(const float4& lo, const float4& hi, const float4& q) {
  return nn_box_lb_f64(nn_gap_f64(lo.x, hi.x, q.x), nn_gap_f64(lo.y, hi.y, q.y), nn_gap_f64(lo.z, hi.z, q.z));
}

// 1-NN of q among the grid's points: *bd = nn_d2, *bi = target index (lowest on ties), *bp = sorted position; (FLT_MAX, -1, -1) when
// nothing is closer than FLT_MAX (empty target, non-finite query), as icp_nn: the pair form's start state (nn_rules.h)
DEV_INLINE void lc_nn(const LcGrid& G, const int* cstart, const float4* cbox, const float4* spts, const float4 q, float* bd_out, int* bi_out, int* bp_out) {
  float bd = FLT_MAX;
  int bi = -1, bp = -1;
  if (G.ncell > 0 && isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
    const float qa[3] = {q.x, q.y, q.z};
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = lc_axis(G, a, qa[a]);
    const int rmax = max(max(G.g[0], G.g[1]), G.g[2]);
    for (int r = 0; r <= rmax; ++r) {
      const int z0 = max(0, c[2] - r), z1 = min(G.g[2] - 1, c[2] + r), y0 = max(0, c[1] - r), y1 = min(G.g[1] - 1, c[1] + r);
      const int x0 = max(0, c[0] - r), x1 = min(G.g[0] - 1, c[0] + r);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          const bool face = abs(z - c[2]) == r || abs(y - c[1]) == r;   // the whole row is on the shell, else only its two ends
          const int xs = face ? 1 : max(1, 2 * r);
          for (int x = face ? x0 : c[0] - r; x <= (face ? x1 : c[0] + r); x += xs) {
            if (x < x0 || x > x1) continue;
            const int cell = nn_lc_index(x, y, z, G.g[0], G.g[1]);
            if (nn_beyond(lc_box_d2(cbox[2 * (size_t)cell], cbox[2 * (size_t)cell + 1], q), bd)) continue;
            for (int j = cstart[cell]; j < cstart[cell + 1]; ++j) {
              const float4 p = spts[j];
              const float d = nn_d2(p.x, p.y, p.z, q.x, q.y, q.z);
              const int idx = __float_as_int(p.w);
              if (nn_better(d, idx, bd, bi)) { bd = d; bi = idx; bp = j; }
            }
          }
        }
      // every unvisited cell lies beyond a face of the visited box: stop when that half-space is farther than the best
      double rb = DBL_MAX;
      bool open = false;
      for (int a = 0; a < 3; ++a) {
        if (c[a] - r - 1 >= 0) { open = true; rb = fmin(rb, nn_face_lb((double)qa[a] - (G.mn[a] + (double)(c[a] - r) * G.h), G.slack[a])); }
        if (c[a] + r + 1 <= G.g[a] - 1) { open = true; rb = fmin(rb, nn_face_lb((G.mn[a] + (double)(c[a] + r + 1) * G.h) - (double)qa[a], G.slack[a])); }
      }
      if (!open || nn_beyond(rb, bd)) break;
    }
  }
  *bd_out = bd; *bi_out = bi; *bp_out = bp;
}

// ---- ICP ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LC_IT) lc_icp(const LcJob* jobs, const LcDet* det, const int* n_tgt, const LcGrid* geo, const int* cstart, const float4* cbox,
                                                const float4* spts, const float4* src, float4* cur, alego_params P, LcOut* out) {
  __shared__ IcpState S;
  __shared__ double s_red[LC_IT / 64][17];
  __shared__ double s_T[17];
  const LcJob J = jobs[blockIdx.x];
  const LcGrid G = geo[blockIdx.x];
  const int ns = det[J.li].n_src, nt = n_tgt[blockIdx.x];
  const float4* sp = src + J.src_off;
  float4* cp = cur + J.src_off;
  const int* cs = cstart + J.cell_off;
  const float4* cb = cbox + 2 * (size_t)J.cell_off;
  const float4* tp = spts + J.raw_off;
  const int tid = threadIdx.x;
  if (tid == 0) {   // icp_init
    for (int k = 0; k < 16; ++k) { S.M[k] = (k % 5 == 0) ? 1.f : 0.f; S.Tf[k] = (k % 5 == 0) ? 1.f : 0.f; }
    S.prev_mse = DBL_MAX; S.fitness = DBL_MAX;
    S.iter = 0; S.done = (ns == 0 || nt == 0) ? 1 : 0; S.converged = 0; S.apply = 0; S.n_src = ns; S.n_tgt = nt;
  }
  for (int i = tid; i < ns; i += LC_IT) cp[i] = sp[i];
  __syncthreads();
  const double max_d2 = P.icp_max_corr_dist * P.icp_max_corr_dist;
  for (int it = 0; it < P.icp_max_iters && !S.done; ++it) {
    float M[12];
    for (int k = 0; k < 12; ++k) M[k] = S.M[k];
    const bool apply = S.apply != 0;
    double v[17];
#pragma unroll
    for (int k = 0; k < 17; ++k) v[k] = 0.0;
    for (int i = tid; i < ns; i += LC_IT) {
      float4 p = cp[i];
      if (apply) {   // transformCloud of the previous iteration (f32), as icp_corr
        const float x = p.x, y = p.y, z = p.z;
        p.x = M[0] * x + M[1] * y + M[2] * z + M[3]; p.y = M[4] * x + M[5] * y + M[6] * z + M[7]; p.z = M[8] * x + M[9] * y + M[10] * z + M[11];
        cp[i] = p;
      }
      float d2;
      int idx, pos;
      lc_nn(G, cs, cb, tp, p, &d2, &idx, &pos);
      if (idx >= 0 && (double)d2 <= max_d2) {
        const float4 q = tp[pos];
        const double a[3] = {p.x, p.y, p.z}, b[3] = {q.x, q.y, q.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) { v[k] += a[k]; v[3 + k] += b[k]; }
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int w = 0; w < 3; ++w) v[6 + u * 3 + w] += a[u] * b[w];
        v[15] += (double)d2; v[16] += 1.0;
      }
    }
#pragma unroll
    for (int k = 0; k < 17; ++k) v[k] = bfly_sum_f64(v[k]);
    if (lane_id() == 0) for (int k = 0; k < 17; ++k) s_red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < 17) { double t = 0; for (int w = 0; w < LC_IT / 64; ++w) t += s_red[w][tid]; s_T[tid] = t; }
    __syncthreads();
    if (tid == 0) icp_update(&S, s_T, P);
    __syncthreads();
  }
  // getFitnessScore(): every source point under final_transformation_ against its nearest target point (no distance limit)
  double s = 0.0, c = 0.0;
  for (int i = tid; i < ns; i += LC_IT) {
    const float4 p0 = sp[i];
    const float* T = S.Tf;
    float4 p;
    p.x = T[0] * p0.x + T[1] * p0.y + T[2] * p0.z + T[3]; p.y = T[4] * p0.x + T[5] * p0.y + T[6] * p0.z + T[7]; p.z = T[8] * p0.x + T[9] * p0.y + T[10] * p0.z + T[11]; p.w = p0.w;
    float d2;
    int idx, pos;
    lc_nn(G, cs, cb, tp, p, &d2, &idx, &pos);
    if (idx >= 0) { s += (double)d2; c += 1.0; }
  }
  s = bfly_sum_f64(s); c = bfly_sum_f64(c);
  if (lane_id() == 0) { s_red[tid >> 6][0] = s; s_red[tid >> 6][1] = c; }
  __syncthreads();
  if (tid == 0) {
    double ts = 0, tc = 0;
    for (int w = 0; w < LC_IT / 64; ++w) { ts += s_red[w][0]; tc += s_red[w][1]; }
    LcOut& o = out[J.li];
    o.converged = S.converged; o.iterations = S.iter; o.n_source = ns; o.n_target = nt;
    o.fitness = (ns && nt && tc > 0) ? ts / tc : DBL_MAX;
    for (int k = 0; k < 16; ++k) o.correction[k] = S.Tf[k];
  }
}

// alego_debug_nn1: the grid of one target, then one thread per query
__global__ void __launch_bounds__(LC_DT) lc_grid_one(const float4* tgt, int n, int cell_cap, LcGrid* geo, int* cstart, int* ccur, float4* cbox, float4* spts) {
  lc_grid_build(tgt, n, cell_cap, geo, cstart, ccur, cbox, spts);
}
__global__ void __launch_bounds__(LC_DT) lc_nn_many(const LcGrid* geo, const int* cstart, const float4* cbox, const float4* spts, const float4* q, int nq, int* idx, float* d2) {
  const int i = blockIdx.x * LC_DT + threadIdx.x;
  if (i >= nq) return;
  const LcGrid G = *geo;
  int pos;
  lc_nn(G, cstart, cbox, spts, q[i], &d2[i], &idx[i], &pos);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#ifndef LC_BUDGET_DEFAULT
#define LC_BUDGET_DEFAULT (1 << 21)   // raw sub-map points per chunk
#endif

struct LcCtx {
  int list_cap = 0;                        // entries per detection pass (the handle's slot count)
  int* list = nullptr;
  LcDet* det = nullptr;
  LcOut* out = nullptr;
  LcJob* jobs = nullptr;
  LcGrid* geo = nullptr;
  int* ntgt = nullptr;
  long long cap = 0;                       // points of every per-chunk region (raw sub-map, source and cells are each planned against it)
  long long budget = LC_BUDGET_DEFAULT;    // chunk budget (ALEGO_LC_BUDGET): chunking never changes a result
  float4 *src = nullptr, *cur = nullptr, *raw = nullptr, *tgt = nullptr, *spts = nullptr, *cbox = nullptr;
  int *cstart = nullptr, *ccur = nullptr;
  VoxCtx V;
  bool vox = false;
  DevPool lists, chunk;                    // own the list arrays (valid while list_cap > 0) and the per-chunk regions (valid while cap > 0)
};

static void lc_free_chunk(LcCtx* C) {
  C->chunk.clear();
  if (C->vox) vox_destroy(&C->V);
  C->vox = false; C->cap = 0;
}
void loop_ctx_destroy(LcCtx* C) {
  if (!C) return;
  lc_free_chunk(C); C->lists.clear();
  delete C;
}
void loop_ctx_set_budget(LcCtx** pc, long long points) {
  if (!*pc) *pc = new LcCtx();
  (*pc)->budget = std::max(1LL, points);
}

// list arrays for list_cap entries; need > 0: per-chunk regions of at least `need` points (+ the VoxelGrid context)
static int lc_reserve(LcCtx* C, int list_cap, long long need, std::string* err) {
  if (C->list_cap < list_cap) {
    C->lists.clear();
    C->list_cap = 0;
    const DevGet get{C->lists, "loop search: ", err};
    if (!get(&C->list, list_cap) || !get(&C->det, list_cap) || !get(&C->out, list_cap) || !get(&C->jobs, list_cap) || !get(&C->geo, list_cap) || !get(&C->ntgt, list_cap)) return ALEGO_ERR_HIP;
    C->list_cap = list_cap;
    if (C->vox) { vox_destroy(&C->V); C->vox = false; }
  }
  if (need > 0 && (C->cap < need || !C->vox)) {
    const long long cap = std::max(C->cap, need);
    lc_free_chunk(C);
    const size_t n = (size_t)cap;
    const DevGet get{C->chunk, "loop search: ", err};
    if (!get(&C->src, n) || !get(&C->cur, n) || !get(&C->raw, n) || !get(&C->tgt, n) || !get(&C->spts, n) || !get(&C->cbox, 2 * n) || !get(&C->cstart, n + 1) || !get(&C->ccur, n + 1)) {
      lc_free_chunk(C); return ALEGO_ERR_HIP;
    }
    // one VoxelGrid job per attempted slot of a chunk; its sort scratch is the slot's region of the raw sub-map (job.off = raw_off)
    std::vector<VoxJob> jz((size_t)C->list_cap);
    std::memset(jz.data(), 0, jz.size() * sizeof(VoxJob));
    jz[0].cap = (int)std::min<long long>(cap, 0x7fffffff);
    if (vox_create(&C->V, jz.data(), (int)jz.size(), err)) { lc_free_chunk(C); return ALEGO_ERR_HIP; }
    C->vox = true;
    C->cap = cap;
  }
  return 0;
}

// The attempts of one piece (det[i].status == 1; C->det holds det already): chunks of consecutive attempts, each gathered by `gather`, then
// VoxelGrid(lc_leaf), lc_grid and lc_icp; o[i] = the verdict on attempt i
static int lc_attempts(LcCtx* C, const alego_params& P, const int* slots, const LcDet* det, int n, const LcGather& gather, LcOut* o, hipStream_t st, std::string* err) {
  // chunks of consecutive attempts whose raw sub-maps, sources and cells fit the budget (a larger single slot grows the scratch)
  const int nfr = 1 + 2 * std::max(0, P.lc_search_num) + 1;
  std::vector<std::vector<LcJob>> chunks;
  std::vector<std::vector<VoxJob>> vjobs;
  long long need = 1;
  {
    std::vector<LcJob> cur;
    long long sr = 0, ss = 0, sc = 0;
    for (int i = 0; i < n; ++i) {
      if (det[i].status != 1) continue;
      const long long r = det[i].n_raw, s = det[i].n_src, c = r / 4 + 2;
      need = std::max(need, std::max(r, std::max(s, c)));
      const long long lim = std::max(C->budget, need);
      if (!cur.empty() && (sr + r > lim || ss + s > lim || sc + c > lim)) { chunks.push_back(cur); cur.clear(); sr = ss = sc = 0; }
      cur.push_back(LcJob{i, slots[i], (int)ss, (int)sr, (int)sc, (int)c});
      sr += r; ss += s; sc += c;
    }
    if (!cur.empty()) chunks.push_back(cur);
  }
  DevTry t("loop search", err);
  if (!chunks.empty()) {
    if (int rc = lc_reserve(C, C->list_cap, std::max(C->budget, need), err)) return rc;
    for (const auto& ch : chunks) {
      const int J = (int)ch.size();
      if (t.up(C->jobs, ch, st)) return t;
      gather(C->jobs, C->det, J, nfr, C->src, C->raw, st);
      vjobs.emplace_back((size_t)J);
      std::vector<VoxJob>& vj = vjobs.back();
      std::memset(vj.data(), 0, vj.size() * sizeof(VoxJob));
      for (int j = 0; j < J; ++j) {
        const LcJob& b = ch[j];
        const int nr = std::max(det[b.li].n_raw, 1);
        vj[j].in = C->raw + b.raw_off; vj[j].n_in = &C->det[b.li].n_raw; vj[j].out = C->tgt + b.raw_off; vj[j].n_out = C->ntgt + j;
        vj[j].leaf = P.lc_leaf; vj[j].cap = nr; vj[j].out_cap = nr; vj[j].off = b.raw_off;
      }
      if (t.up(C->V.jobs, vj, st)) return t;
      VoxCtx V = C->V;
      V.njobs = J; V.grid_small = J; V.grid_big = J;
      if (int rc = vox_run(V, st, err)) return rc;
      ALEGO_LAUNCH(lc_grid, dim3(J), dim3(LC_DT), 0, st, C->jobs, C->ntgt, C->tgt, C->geo, C->cstart, C->ccur, C->cbox, C->spts);
      ALEGO_LAUNCH(lc_icp, dim3(J), dim3(LC_IT), 0, st, C->jobs, C->det, C->ntgt, C->geo, C->cstart, C->cbox, C->spts, C->src, C->cur, P, C->out);
      // the next chunk reuses jobs / scratch: the copies and kernels above are ordered on `st`
    }
  }
  return t.at("kernels").down(o, C->out, (size_t)n, st).wait(st);
}

// one piece of the list (at most list_cap entries): detection, then the attempted slots in chunks
static int lc_piece(LcCtx* C, const LmCtx& L, const alego_params& P, const int* slots, int n, alego_loop_result* res, hipStream_t st, std::string* err) {
  DevTry t("loop search", err);
  if (t.up(C->list, slots, (size_t)n, st)) return t;
  ALEGO_LAUNCH(lc_detect, dim3(n), dim3(LC_DT), 0, st, L, C->list, P, C->det);
  std::vector<LcDet> det((size_t)n);
  if (t.at("detection").down(det, C->det, st).wait(st)) return t;
  std::vector<LcOut> o((size_t)n);
  if (int rc = lc_attempts(C, P, slots, det.data(), n, loop_archive_gather(L), o.data(), st, err)) return rc;
  for (int i = 0; i < n; ++i) {
    alego_loop_result& r = res[i];
    std::memset(&r, 0, sizeof(r));
    const LcDet& D = det[i];
    r.status = D.status; r.latest_id = D.latest; r.closest_id = D.closest;
    if (D.status == 1) loop_result_fill(D, o[i], P.lc_fitness_max, &r);
  }
  return 0;
}

LcGather loop_archive_gather(const LmCtx& L) {   // (L outlives the attempts it is handed to)
  return [&L](const LcJob* jobs, const LcDet* dd, int J, int nfr, float4* src, float4* raw, hipStream_t s2) {
    ALEGO_LAUNCH(lc_gather, dim3(nfr, J), dim3(LC_DT), 0, s2, L, jobs, dd, src, raw);
  };
}

bool loop_result_fill(const LcDet& D, const LcOut& O, double fitness_max, alego_loop_result* r) {
  r->closest_id = D.closest;
  r->converged = O.converged; r->iterations = O.iterations; r->n_source = O.n_source; r->n_target = O.n_target;
  r->fitness = O.fitness;
  for (int k = 0; k < 16; ++k) r->correction[k] = O.correction[k];
  r->status = (O.converged && O.fitness <= fitness_max) ? 2 : 1;   // :697
  alego_loop_constraint(r->correction, D.pose_latest, D.pose_closest, r->t_correct, r->between);
  r->noise_variance = (double)(float)O.fitness;
  return r->status == 2;
}

int loop_search(LcCtx** pc, const LmCtx& L, const alego_params& P, int n_slots, const int* slots, int n, alego_loop_result* res, hipStream_t st, std::string* err) {
  if (!*pc) *pc = new LcCtx();
  LcCtx* C = *pc;
  if (int rc = lc_reserve(C, n_slots, 0, err)) return rc;
  for (int i0 = 0; i0 < n; i0 += C->list_cap)
    if (int rc = lc_piece(C, L, P, slots + i0, std::min(C->list_cap, n - i0), res + i0, st, err)) return rc;
  return 0;
}

int loop_attempts(LcCtx** pc, const alego_params& P, int n_slots, const int* slots, const LcDet* det, int n, const LcGather& gather, LcOut* out, hipStream_t st, std::string* err) {
  if (!*pc) *pc = new LcCtx();
  LcCtx* C = *pc;
  if (int rc = lc_reserve(C, n_slots, 0, err)) return rc;
  if (n <= 0) return lc_attempts(C, P, slots, det, 0, gather, out, st, err);
  // pieces of list_cap entries (>= n_slots: the list arrays only grow): every list array and scratch region is keyed by entry or job, none by slot, so
  // entries may repeat a slot
  for (int i0 = 0; i0 < n; i0 += C->list_cap) {
    const int c = std::min(C->list_cap, n - i0);
    if (int rc = DevTry("loop attempts", err).up(C->det, det + i0, (size_t)c, st)) return rc;
    if (int rc = lc_attempts(C, P, slots + i0, det + i0, c, gather, out + i0, st, err)) return rc;
  }
  return 0;
}

int loop_rounds(LcCtx** pc, const alego_params& P, int n_slots, const int* slots, int n, int rounds, const LcGather& gather, const LcPlan& plan, const LcVerdict& verdict, hipStream_t st,
                std::string* err) {
  std::vector<LcDet> det((size_t)n);
  std::vector<LcOut> res((size_t)n);
  std::vector<char> accepted((size_t)n, 0);
  for (int v = 0; v < rounds; ++v) {
    bool any = false;
    for (int i = 0; i < n; ++i) {
      std::memset(&det[i], 0, sizeof(LcDet));
      const bool go = !accepted[i] && plan(i, v, &det[i]);
      det[i].status = go ? 1 : 0;
      any = any || go;
    }
    if (!any) break;   // nothing left to try
    if (int rc = loop_attempts(pc, P, n_slots, slots, det.data(), n, gather, res.data(), st, err)) return rc;
    for (int i = 0; i < n; ++i)
      if (det[i].status == 1) accepted[i] = verdict(i, v, det[i], res[i]);
  }
  return 0;
}

int loop_debug_nn1(const alego_point* tgt, int n_tgt, const alego_point* q, int nq, int32_t* idx, float* d2, hipStream_t st, std::string* err) {
  DevPool tmp;   // temporaries of this call
  auto get = [&](auto** p, size_t count) { return tmp.get(p, count, false) == hipSuccess; };
  const int cell_cap = n_tgt / 4 + 2;
  float4 *dt, *dq, *sp, *cb; int *cs, *cc, *di; float* dd; LcGrid* g;
  if (!get(&dt, (size_t)n_tgt) || !get(&dq, (size_t)nq) || !get(&sp, (size_t)n_tgt) || !get(&cb, (size_t)cell_cap * 2) ||
      !get(&cs, (size_t)cell_cap + 1) || !get(&cc, (size_t)cell_cap + 1) || !get(&di, (size_t)nq) || !get(&dd, (size_t)nq) ||
      !get(&g, 1)) { *err = "debug_nn1: allocation failed"; return ALEGO_ERR_HIP; }
  DevTry c("debug_nn1", err);
  if (c.up(dt, tgt, (size_t)n_tgt, st).up(dq, q, (size_t)nq, st)) return c;
  ALEGO_LAUNCH(lc_grid_one, dim3(1), dim3(LC_DT), 0, st, dt, n_tgt, cell_cap, g, cs, cc, cb, sp);
  if (nq) ALEGO_LAUNCH(lc_nn_many, dim3((nq + LC_DT - 1) / LC_DT), dim3(LC_DT), 0, st, g, cs, cb, sp, dq, nq, di, dd);
  return c.down(idx, di, (size_t)nq, st).down(d2, dd, (size_t)nq, st).wait(st);
}
