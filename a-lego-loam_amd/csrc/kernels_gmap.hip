// kernels_gmap.hip — the global map (saveMapCB, laserMapping.cpp:826-874; visualizeGlobalMapThread, :598-631) on gfx950.
//
//   map_archive        appends the key frame lm_store_kf just wrote (sensor-frame clouds + f32 key pose + stamp) to the slot's archive
//   map_offsets        exclusive prefix sum of the selected cloud sizes of the archived frames (one workgroup per slot)
//   map_gather         every selected point transformed by its frame's archived key pose (transformPointCloud,
//                      laserMapping.h:164-186), written once at its offset
//   gv_*               pcl::VoxelGrid over a cloud of any size spread over the whole chip (vox_big, kernels_voxel.hip, sorts one
//                      cloud inside one workgroup and is the right tool only for the local maps' 45-75 k points):
//                        gv_bbox     getMinMax3D as a multi-workgroup min / max (order-preserving u32 codes, atomicMin)
//                        gv_geom     one thread: minb, divb, PCL's dx dy dz > INT_MAX pass-through rule, radix pass count
//                        gv_keys     voxel key per point (PCL's arithmetic, 32-bit int), point index
//                        gv_hist / gs_* / gv_scatter   one stable LSD radix pass over (key, index): per-tile digit histogram,
//                                    device-wide exclusive scan (digit-major, so tiles keep their order), stable scatter —
//                                    the phases are separated by kernel boundaries, no workgroup ever waits for another
//                        gv_flags / gs_* / gv_starts   run heads of the sorted keys, compacted by a scan
//                        gv_sum      one thread per voxel: f32 sums in sorted (= input) order, divided by the count
//                        gv_copy     the pass-through case: output = input, in input order
//   Every launch is sized by the host's n; passes the geometry does not need return at once (no host round trip).
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "../../include/alego_mi355x.h"
#include "dev_copy.h"
#include "gmap.h"
#include "kf_store.h"
#include "pg_math.h"
#include "prof.h"
#include "vgrid.h"

#define GM_T 256
#define GS_T 1024                    // scan workgroup
#define GS_PER 4                     // elements per thread of a scan workgroup
#define GS_BLK (GS_T * GS_PER)
#define GV_T 256                     // radix workgroup = one digit per thread
#define GV_D 8                       // digit width
#define GV_ND (1 << GV_D)
#define GV_TILE 4096                 // elements per radix tile (16 rounds of 256)
#define GV_MAXP 4                    // 32-bit keys

enum { GG_MINB = 0, GG_MUL1 = 3, GG_MUL2 = 4, GG_PASS = 5, GG_P = 6 };

// ---- archive ------------------------------------------------------------------------------------------------------
// grid (slots of the launch), GM_T threads: a frame that does not fit (frames or points) is dropped whole and counted; after the
// first drop every later frame is dropped too, so the stored frames stay a prefix of the key-frame ids
__global__ void __launch_bounds__(GM_T) map_archive(DevCtx d, LmCtx L, int force) {
  const int slot = blockIdx.x + d.slot0;
  const int* li = L.li + (size_t)slot * LI_COUNT;
  if (!force && !li[LI_KF_ADDED]) return;
  const KfRingRow R = kf_ring_row_at(L, slot, kf_entry(L, li[LI_NKF] - 1), KF_CORNER);
  const int nc = R.cnt[KF_CORNER], ns = R.cnt[KF_SURF], no = R.cnt[KF_OUTL];
  int* st = arc_stat_of(L, slot);
  const int nf = st[AS_FRAMES], dropped = st[AS_DROPPED], np = st[AS_POINTS];
  const bool fits = dropped == 0 && nf < L.arc_frames_cap && (long long)np + nc + ns + no <= (long long)L.arc_points_cap;
  __syncthreads();   // every thread has read the counters before thread 0 moves them
  if (!fits) {
    if (threadIdx.x == 0) st[AS_DROPPED] = dropped + 1;
    return;
  }
  float4* dst = L.arc_pts + (size_t)slot * L.arc_points_cap + np;
  const float4 *rc = R.raw, *rsf = kf_raw_of(L, R.row, KF_SURF), *ro = kf_raw_of(L, R.row, KF_OUTL);
  for (int i = threadIdx.x; i < nc + ns + no; i += GM_T) dst[i] = i < nc ? rc[i] : (i < nc + ns ? rsf[i - nc] : ro[i - nc - ns]);
  if (threadIdx.x < KF_POSE_W) arc_pose_of(L, slot, nf)[threadIdx.x] = R.pose[threadIdx.x];
  if (threadIdx.x == 0) {
    int* tab = arc_tab_of(L, slot, nf);
    tab[AT_OFF] = np; tab[AT_N + KF_CORNER] = nc; tab[AT_N + KF_SURF] = ns; tab[AT_N + KF_OUTL] = no;
    // the stamp of the scan that saved the frame; paths without stamps (batch, replay) number the slot's mapping frames
    L.arc_stamp[arc_row(L, slot, nf)] = L.arc_stamped[slot] ? d.scan_stamp[slot] : (double)(li[LI_FRAME] - 1) * d.P.scan_period;
    st[AS_FRAMES] = nf + 1; st[AS_POINTS] = np + nc + ns + no;
    // the key-pose graph (alego_graph_enable): PriorFactor on the first frame (:495), else BetweenFactor(pre_pose, this pose) (:510-512),
    // both poses as Pose3(Rot3::RzRyRx, xyz) of their f32 key poses; pre_pose is the archived pose of frame nf - 1 as it stands now
    if (L.pg_loops_cap > 0) {
      alego_graph_edge* e = L.pg_chain + arc_row(L, slot, nf);
      double xn[12];
      pg_from_pose6(R.pose, xn);
      e->from = nf - 1; e->to = nf;
      if (nf == 0) {
        for (int k = 0; k < 12; ++k) e->between[k] = xn[k];
      } else {
        double xp[12];
        pg_from_pose6(arc_pose_of(L, slot, nf - 1), xp);
        pg_between(xp, xn, e->between);
      }
      for (int k = 0; k < 6; ++k) e->variance[k] = L.pg_odom_var[k];
      // alego_regcov_enable with graph = 1: an odometry edge of a frame the registration itself saved carries that registration's variances (the
      // newer frame's covariance alone, in its tangent space); the prior, a forced archive and a record without a result keep pg_odom_var
      if (L.rc_graph && !force && nf > 0) {
        const alego_regcov* rc = L.rc_rec + slot;
        if (rc->status == 1 && rc->frame == li[LI_FRAME]) for (int k = 0; k < 6; ++k) e->variance[k] = rc->variance[k];
      }
    }
  }
}

void launch_map_archive(const DevCtx& d, const LmCtx& L, int force, hipStream_t st) {
  ALEGO_LAUNCH(map_archive, dim3(d.n_launch), dim3(GM_T), 0, st, d, L, force);
}

// ---- assembly -----------------------------------------------------------------------------------------------------
// one workgroup: off[f] = selected points of frames [0, f), off[nf] = *n = the total
__global__ void __launch_bounds__(GS_T) map_offsets(LmCtx L, int slot, int nf, int kinds, int* off, int* n) {
  __shared__ int s_w[17];
  int carry = 0;
  for (int f0 = 0; f0 < nf; f0 += GS_T) {
    const int f = f0 + threadIdx.x;
    const int v = f < nf ? kf_sel_count(kf_arc_frame(L, slot, f), kinds) : 0;
    int tot;
    const int ex = block_excl_scan<GS_T / 64>(v, s_w, &tot);
    if (f < nf) off[f] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) { off[nf] = carry; *n = carry; }
}

// grid (frames): within a frame surf, corner, outlier (visualizeGlobalMapThread :607-612), restricted to `kinds`; kinds & 8: intensity =
// frame index (transformPointCloud(cloud, pose, idx), laserMapping.h:178-186)
__global__ void __launch_bounds__(GM_T) map_gather(LmCtx L, int slot, int kinds, const int* off, float4* out) {
  const int f = blockIdx.x;
  const KfArcFrame A = kf_arc_frame(L, slot, f);
  const int n = kf_sel_count(A, kinds);
  float m[3][4];
  keypose_matrix(A.pose, m);
  float4* dst = out + off[f];
  const float fid = (float)f;
  for (int i = threadIdx.x; i < n; i += GM_T) {
    float4 p = kf_transform(m, A.pts[kf_arc_index(A.nc, A.ns, kinds, i)]);
    if (kinds & 8) p.w = fid;
    dst[i] = p;
  }
}

void launch_map_offsets(const LmCtx& L, int slot, int nf, int kinds, int* off, int* n_dev, hipStream_t st) {
  ALEGO_LAUNCH(map_offsets, dim3(1), dim3(GS_T), 0, st, L, slot, nf, kinds, off, n_dev);
}
void launch_map_assemble(const LmCtx& L, int slot, int nf, int kinds, float4* out, int* off_scratch, int* n_dev, hipStream_t st) {
  launch_map_offsets(L, slot, nf, kinds, off_scratch, n_dev, st);
  if (nf > 0) ALEGO_LAUNCH(map_gather, dim3(nf), dim3(GM_T), 0, st, L, slot, kinds, off_scratch, out);
}

// ---- device-wide exclusive scan (in place) ------------------------------------------------------------------------
__global__ void __launch_bounds__(GS_T) gs_block(int* a, int n, int* bs) {
  __shared__ int s_w[17];
  const size_t base = (size_t)blockIdx.x * GS_BLK + (size_t)threadIdx.x * GS_PER;
  int v[GS_PER], s = 0;
#pragma unroll
  for (int k = 0; k < GS_PER; ++k) { v[k] = base + k < (size_t)n ? a[base + k] : 0; s += v[k]; }
  int tot;
  int run = block_excl_scan<GS_T / 64>(s, s_w, &tot);
#pragma unroll
  for (int k = 0; k < GS_PER; ++k) { if (base + k < (size_t)n) a[base + k] = run; run += v[k]; }
  if (threadIdx.x == 0) bs[blockIdx.x] = tot;
}
// one workgroup: exclusive scan of the nb block sums, chunk by chunk
__global__ void __launch_bounds__(GS_T) gs_top(int* bs, int nb) {
  __shared__ int s_w[17];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += GS_T) {
    const int b = b0 + threadIdx.x;
    const int v = b < nb ? bs[b] : 0;
    int tot;
    const int ex = block_excl_scan<GS_T / 64>(v, s_w, &tot);
    if (b < nb) bs[b] = carry + ex;
    carry += tot;
  }
}
__global__ void __launch_bounds__(GS_T) gs_add(int* a, int n, const int* bs) {
  const int add = bs[blockIdx.x];
  const size_t base = (size_t)blockIdx.x * GS_BLK;
  for (int k = threadIdx.x; k < GS_BLK; k += GS_T) if (base + k < (size_t)n) a[base + k] += add;
}
static void scan_excl(int* a, int n, int* bs, hipStream_t st) {
  const int nb = (n + GS_BLK - 1) / GS_BLK;
  ALEGO_LAUNCH(gs_block, dim3(nb), dim3(GS_T), 0, st, a, n, bs);
  ALEGO_LAUNCH(gs_top, dim3(1), dim3(GS_T), 0, st, bs, nb);
  ALEGO_LAUNCH(gs_add, dim3(nb), dim3(GS_T), 0, st, a, n, bs);
}

// ---- device-wide VoxelGrid ----------------------------------------------------------------------------------------
// getMinMax3D: per-lane fminf / fmaxf, wavefront shuffles, one atomicMin per workgroup and axis on the order-preserving codes (vgrid.h)
__global__ void __launch_bounds__(GV_T) gv_bbox(const float4* in, int n, unsigned* bbox) {
  __shared__ float s_r[6][GV_T / 64];
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (size_t i = (size_t)blockIdx.x * GV_T + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * GV_T) vgr_box_add(mn, mx, in[i]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bfly_minmax_f32(mn[a], mx[a]);
    if (lane == 0) { s_r[a][wave] = mn[a]; s_r[3 + a][wave] = mx[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = s_r[a][0];
    for (int w = 1; w < GV_T / 64; ++w) v = a < 3 ? fminf(v, s_r[a][w]) : fmaxf(v, s_r[a][w]);
    if (a < 3) atomicMin(bbox + a, vgr_enc(v));
    else atomicMin(bbox + 1 + a, ~vgr_enc(v));
  }
}

// one thread: the grid geometry exactly as vox_big / oracle voxel_grid derive it
__global__ void gv_geom(const unsigned* bbox, float leaf, int* geom) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float inv = 1.0f / leaf;
  float mn[3], mx[3];
  vgr_box_load(bbox, mn, mx);
  if (vgr_leaf_too_small(mn, mx, inv)) { geom[GG_PASS] = 1; geom[GG_P] = 0; return; }   // PCL: "leaf size too small" -> output = input
  const VgrGeom g = vgr_geom(mn, mx, inv);
  for (int a = 0; a < 3; ++a) geom[GG_MINB + a] = g.minb[a];
  geom[GG_MUL1] = (int)g.mul1;
  geom[GG_MUL2] = (int)g.mul2;
  geom[GG_PASS] = 0;
  geom[GG_P] = (vgr_bits(g.T) + GV_D - 1) / GV_D;
}

__global__ void __launch_bounds__(GV_T) gv_keys(const float4* in, int n, float leaf, const int* geom, unsigned* keys, int* vals) {
  if (geom[GG_PASS]) return;
  const float inv = 1.0f / leaf;
  VgrGeom g;
  for (int a = 0; a < 3; ++a) g.minb[a] = geom[GG_MINB + a];
  g.mul1 = (unsigned)geom[GG_MUL1];
  g.mul2 = (unsigned)geom[GG_MUL2];
  for (size_t i = (size_t)blockIdx.x * GV_T + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * GV_T) {
    keys[i] = vgr_id(g, in[i], inv);
    vals[i] = (int)i;
  }
}

// grid (tiles): digit counts of tile t at hist[digit * tiles + t]
__global__ void __launch_bounds__(GV_T) gv_hist(const unsigned* keys, int n, int pass, const int* geom, int* hist) {
  if (pass >= geom[GG_P]) return;
  __shared__ int s_c[GV_ND];
  s_c[threadIdx.x] = 0;
  __syncthreads();
  const int sh = pass * GV_D;
  const size_t base = (size_t)blockIdx.x * GV_TILE;
  for (int k = threadIdx.x; k < GV_TILE; k += GV_T) if (base + k < (size_t)n) atomicAdd(&s_c[(keys[base + k] >> sh) & (GV_ND - 1)], 1);
  __syncthreads();
  hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s_c[threadIdx.x];
}

// grid (tiles): the tile's elements in order, 256 at a time; the rank among equal digits of a wavefront comes from 8 ballots (lanes are in
// index order), wavefronts of lower index and earlier rounds come first — a stable scatter
__global__ void __launch_bounds__(GV_T) gv_scatter(const unsigned* ks, const int* vs, unsigned* kd, int* vd, int n, int pass, const int* geom, const int* hist) {
  if (pass >= geom[GG_P]) return;
  __shared__ int s_run[GV_ND];
  __shared__ int s_wc[GV_T / 64][GV_ND];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sh = pass * GV_D;
  s_run[tid] = hist[(size_t)tid * gridDim.x + blockIdx.x];
  const size_t base = (size_t)blockIdx.x * GV_TILE;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = 0; r < GV_TILE; r += GV_T) {
#pragma unroll
    for (int w = 0; w < GV_T / 64; ++w) s_wc[w][tid] = 0;
    const size_t i = base + r + tid;
    const bool ok = i < (size_t)n;
    const unsigned key = ok ? ks[i] : 0u;
    const int val = ok ? vs[i] : 0;
    const int dg = (int)((key >> sh) & (GV_ND - 1));
    unsigned long long m = __ballot(ok);
#pragma unroll
    for (int b = 0; b < GV_D; ++b) {
      const unsigned long long bb = __ballot((dg >> b) & 1);
      m &= ((dg >> b) & 1) ? bb : ~bb;
    }
    const int rank = __popcll(m & lt);
    __syncthreads();   // (s_wc cleared; s_run of the previous round updated)
    if (ok && rank == 0) s_wc[wave][dg] = __popcll(m);
    __syncthreads();
    if (ok) {
      int pos = s_run[dg] + rank;
      for (int w = 0; w < wave; ++w) pos += s_wc[w][dg];
      kd[pos] = key; vd[pos] = val;
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < GV_T / 64; ++w) add += s_wc[w][tid];
    s_run[tid] += add;
    __syncthreads();
  }
}

DEV_INLINE const unsigned* gv_final_keys(const int* geom, const unsigned* kA, const unsigned* kB) { return (geom[GG_P] & 1) ? kB : kA; }

__global__ void __launch_bounds__(GV_T) gv_flags(const unsigned* kA, const unsigned* kB, int n, const int* geom, int* run) {
  if (geom[GG_PASS]) return;
  const unsigned* k = gv_final_keys(geom, kA, kB);
  for (size_t i = (size_t)blockIdx.x * GV_T + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * GV_T) run[i] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0;
}
// run[] holds the exclusive scan of the head flags: starts[rank] = position of every head, starts[voxels] = n, cnt[1] = voxels
__global__ void __launch_bounds__(GV_T) gv_starts(const unsigned* kA, const unsigned* kB, int n, const int* geom, const int* run, int* starts, int* cnt) {
  if (geom[GG_PASS]) return;
  const unsigned* k = gv_final_keys(geom, kA, kB);
  for (size_t i = (size_t)blockIdx.x * GV_T + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * GV_T) {
    const bool head = i == 0 || k[i] != k[i - 1];
    if (head) starts[run[i]] = (int)i;
    if (i == (size_t)n - 1) { const int nv = run[i] + (head ? 1 : 0); starts[nv] = n; cnt[1] = nv; }
  }
}
// one thread per voxel (pcl::CentroidPoint: f32 sums in sorted order, divided by the count), four gathers in flight
__global__ void __launch_bounds__(GV_T) gv_sum(const float4* in, const int* vA, const int* vB, const int* geom, const int* starts, const int* cnt, float4* out) {
  if (geom[GG_PASS]) return;
  const int* v = (geom[GG_P] & 1) ? vB : vA;
  const int nv = cnt[1];
  for (int r = blockIdx.x * GV_T + threadIdx.x; r < nv; r += gridDim.x * GV_T) {
    const int a = starts[r], b = starts[r + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    for (int j = a; j < b; j += 4) {
      float4 pt[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) pt[q] = in[v[min(j + q, b - 1)]];
#pragma unroll
      for (int q = 0; q < 4; ++q) if (j + q < b) { sx += pt[q].x; sy += pt[q].y; sz += pt[q].z; si += pt[q].w; }
    }
    const float fn = (float)(b - a);
    out[r] = make_float4(sx / fn, sy / fn, sz / fn, si / fn);
  }
}
__global__ void __launch_bounds__(GV_T) gv_copy(const float4* in, int n, const int* geom, float4* out, int* cnt) {
  if (!geom[GG_PASS]) return;
  for (size_t i = (size_t)blockIdx.x * GV_T + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * GV_T) out[i] = in[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[1] = n;
}

// ---- host ---------------------------------------------------------------------------------------------------------
void gv_destroy(GvCtx* G) {
  vox_destroy(&G->small);
  G->mem.clear();
  G->cap = 0; G->small_cap = 0;
}

int gv_reserve(GvCtx* G, int n, std::string* err) {
  if (n <= G->cap && G->cap > 0) return 0;
  const int keep_small = G->small_max;
  gv_destroy(G);
  *G = GvCtx();
  G->small_max = keep_small;
  const int cap = std::max(n, 1);
  const size_t tiles = ((size_t)cap + GV_TILE - 1) / GV_TILE;
  const size_t hist_n = tiles * GV_ND;
  const size_t bs_n = std::max(hist_n, (size_t)cap) / GS_BLK + 1;
  hipError_t e = hipSuccess;
  auto A = [&](auto** p, size_t count) { if (e == hipSuccess) e = G->mem.get(p, count, false); };
  A(&G->in, cap); A(&G->out, cap); A(&G->kA, cap); A(&G->kB, cap); A(&G->vA, cap); A(&G->vB, cap);
  A(&G->run, cap); A(&G->starts, (size_t)cap + 1); A(&G->hist, hist_n); A(&G->bsum, bs_n);
  A(&G->bbox, 8); A(&G->geom, 16); A(&G->cnt, 2);
  if (e == hipSuccess) e = hipMemset(G->geom, 0, 16 * sizeof(int));
  if (e != hipSuccess) { *err = std::string("voxel grid scratch: ") + hipGetErrorString(e); gv_destroy(G); return -2; }
  // the one-workgroup path over the same buffers, for clouds up to small_max points
  G->small_cap = std::max(1, std::min(cap, G->small_max));
  VoxJob job{G->in, G->cnt, G->out, G->cnt + 1, nullptr, 1.0f, G->small_cap, G->small_cap, nullptr, 0};
  if (vox_create(&G->small, &job, 1, err)) { gv_destroy(G); return -2; }
  G->cap = cap;
  return 0;
}

int gv_filter(GvCtx* G, int n, float leaf, hipStream_t st, std::string* err) {
  if (n <= 0) return hipMemsetAsync(G->cnt + 1, 0, sizeof(int), st) == hipSuccess ? 0 : -2;
  if (n > G->cap) { *err = "voxel grid: scratch too small"; return -3; }
  if (n <= G->small_cap && n <= G->small_max) {
    // (the job table lives on the device: only its leaf changes between calls)
    static_assert(std::is_same<decltype(VoxJob::leaf), float>::value && ALEGO_ERR_HIP == -2, "the leaf of a job is one float; a failed copy returns this file's -2");
    float* leaf_dev = reinterpret_cast<float*>(reinterpret_cast<char*>(G->small.jobs) + offsetof(VoxJob, leaf));
    if (int r = DevTry("voxel grid", err, "job upload").up(leaf_dev, &leaf, 1, st).wait(st)) return r;
    return vox_run(G->small, st, err);
  }
  const int nb = (int)std::min<size_t>(((size_t)n + GV_T * 8 - 1) / (GV_T * 8), 2048);
  const int tiles = (int)(((size_t)n + GV_TILE - 1) / GV_TILE);
  if (hipMemsetAsync(G->bbox, 0xFF, 8 * sizeof(unsigned), st) != hipSuccess) { *err = "voxel grid: memset failed"; return -2; }
  ALEGO_LAUNCH(gv_bbox, dim3(nb), dim3(GV_T), 0, st, G->in, n, G->bbox);
  ALEGO_LAUNCH(gv_geom, dim3(1), dim3(64), 0, st, G->bbox, leaf, G->geom);
  ALEGO_LAUNCH(gv_keys, dim3(nb), dim3(GV_T), 0, st, G->in, n, leaf, G->geom, G->kA, G->vA);
  for (int p = 0; p < GV_MAXP; ++p) {   // passes beyond the geometry's (gv_geom) return at once
    const unsigned* ks = (p & 1) ? G->kB : G->kA;
    const int* vs = (p & 1) ? G->vB : G->vA;
    unsigned* kd = (p & 1) ? G->kA : G->kB;
    int* vd = (p & 1) ? G->vA : G->vB;
    ALEGO_LAUNCH(gv_hist, dim3(tiles), dim3(GV_T), 0, st, ks, n, p, G->geom, G->hist);
    scan_excl(G->hist, tiles * GV_ND, G->bsum, st);
    ALEGO_LAUNCH(gv_scatter, dim3(tiles), dim3(GV_T), 0, st, ks, vs, kd, vd, n, p, G->geom, G->hist);
  }
  ALEGO_LAUNCH(gv_flags, dim3(nb), dim3(GV_T), 0, st, G->kA, G->kB, n, G->geom, G->run);
  scan_excl(G->run, n, G->bsum, st);
  ALEGO_LAUNCH(gv_starts, dim3(nb), dim3(GV_T), 0, st, G->kA, G->kB, n, G->geom, G->run, G->starts, G->cnt);
  ALEGO_LAUNCH(gv_sum, dim3(nb), dim3(GV_T), 0, st, G->in, G->vA, G->vB, G->geom, G->starts, G->cnt, G->out);
  ALEGO_LAUNCH(gv_copy, dim3(nb), dim3(GV_T), 0, st, G->in, n, G->geom, G->out, G->cnt);
  return 0;
}

int gv_small_max_env() {
  const char* e = getenv("ALEGO_GV_SMALL_MAX");
  return e ? std::max(0, atoi(e)) : GV_SMALL_MAX_DEFAULT;
}
