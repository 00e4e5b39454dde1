// kernels_icp.hip — the numeric part of loop closure (src/laserMapping.cpp:652-824): sub-map assembly of detectLoopClosure
// (:794-812) and pcl::IterativeClosestPoint as performLoopClosure configures it (:670-692).  The pose graph (GTSAM) and the
// decision logic stay on the host (alego_loop_detect is a host helper); this is the per-point work.
//
//   icp_build     transformPointCloud of the newest key frame (source: surf, corner, outlier) and of the history frames (raw target)
//   (voxel.h)     VoxelGrid(lc_leaf) of the raw target -> near_history_keyframes_
//   icp_corr      one thread per source point: apply the last iteration's transformation (f32, as pcl::transformPointCloud), exact
//                 1-NN in the target (f32 squared distance, ties -> lowest index; target tiled through LDS), correspondences within the
//                 maximum distance feed the sums of the closed-form alignment (f64): per-workgroup partials in fixed order
//   icp_step      one workgroup: partials -> sums, then (icp_math.h) Horn's closed-form rigid transform (largest eigenvector of the 4x4 quaternion
//                 matrix; PCL's TransformationEstimationSVD solves the same least-squares problem by SVD in f32), accumulation of
//                 final_transformation_ (Matrix4f), DefaultConvergenceCriteria (iterations, transformation epsilon, absolute and
//                 relative MSE)
//   icp_fitness   getFitnessScore(): mean squared distance of the source under the final transformation to its nearest target point
// The host enqueues icp_max_iters x (icp_corr, icp_step); kernels of a finished alignment return at once.
#include <vector>

#include "dev_common.h"
#include "kf_store.h"
#include "nn_rules.h"
#include "prof.h"
#include "voxel.h"
#include "icp_math.h"

#define ICP_T 256
#define ICP_TILE 2048

struct IcpFrame { float pose[6]; int off[4]; int dst[3]; };   // raw cloud offsets (corner, surf, outlier, end) and destination offsets of the three clouds

__global__ void __launch_bounds__(ICP_T) icp_build(const IcpFrame* frames, int nframes, const float4* raw, float4* src, float4* tgt_raw) {
  const int f = blockIdx.y;
  const IcpFrame F = frames[f];
  float m[3][4];
  float kp[8] = {F.pose[0], F.pose[1], F.pose[2], F.pose[3], F.pose[4], F.pose[5], 0.f, 0.f};
  keypose_matrix(kp, m);
  float4* dst = f == 0 ? src : tgt_raw;
  for (int kind = 0; kind < 3; ++kind) {
    const int n = F.off[kind + 1] - F.off[kind];
    for (int i = blockIdx.x * ICP_T + threadIdx.x; i < n; i += gridDim.x * ICP_T) dst[F.dst[kind] + i] = kf_transform(m, raw[F.off[kind] + i]);
  }
}

// exact 1-NN of p in tgt[0..n): nn_d2, ties -> lowest index, from the pair form's start state (nn_rules.h); the target goes through LDS in tiles
DEV_INLINE void icp_nn(const float4 p, const float4* tgt, int n, float4* s_tile, float* best_d, int* best_i) {
  float bd = FLT_MAX;
  int bi = -1;
  for (int t0 = 0; t0 < n; t0 += ICP_TILE) {
    const int m = min(ICP_TILE, n - t0);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += ICP_T) s_tile[j] = tgt[t0 + j];
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const float4 q = s_tile[j];
      const float r = nn_d2(q.x, q.y, q.z, p.x, p.y, p.z);
      if (r < bd) { bd = r; bi = t0 + j; }   // nn_better for candidates in ascending index: its tie term is never true
    }
  }
  *best_d = bd; *best_i = bi;
}

// grid ceil(n_src / ICP_T); partial[wg][18]: 15 sums, mse sum, count
__global__ void __launch_bounds__(ICP_T) icp_corr(IcpState* S, float4* cur, const float4* tgt, double max_d2, double* partial) {
  if (S->done) return;
  __shared__ float4 s_tile[ICP_TILE];
  __shared__ double s_red[ICP_T / 64][17];
  const int n_src = S->n_src, n_tgt = S->n_tgt;
  const int i = blockIdx.x * ICP_T + threadIdx.x;
  float4 p = cur[min(i, n_src - 1)];
  if (S->apply) {   // transformCloud of the previous iteration (f32)
    const float* M = S->M;
    const float x = p.x, y = p.y, z = p.z;
    p.x = M[0] * x + M[1] * y + M[2] * z + M[3]; p.y = M[4] * x + M[5] * y + M[6] * z + M[7]; p.z = M[8] * x + M[9] * y + M[10] * z + M[11];
    if (i < n_src) cur[i] = p;
  }
  float d2;
  int idx;
  icp_nn(p, tgt, n_tgt, s_tile, &d2, &idx);
  double v[17];
#pragma unroll
  for (int k = 0; k < 17; ++k) v[k] = 0.0;
  if (i < n_src && idx >= 0 && (double)d2 <= max_d2) {
    const float4 q = tgt[idx];
    const double a[3] = {p.x, p.y, p.z}, b[3] = {q.x, q.y, q.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) { v[k] = a[k]; v[3 + k] = b[k]; }
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int w = 0; w < 3; ++w) v[6 + u * 3 + w] = a[u] * b[w];
    v[15] = (double)d2; v[16] = 1.0;
  }
#pragma unroll
  for (int k = 0; k < 17; ++k) v[k] = bfly_sum_f64(v[k]);
  if (lane_id() == 0) for (int k = 0; k < 17; ++k) s_red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 17) {
    double t = 0;
    for (int w = 0; w < ICP_T / 64; ++w) t += s_red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * 18 + threadIdx.x] = t;
  }
}

__global__ void icp_step(IcpState* S, const double* partial, int nwg, alego_params P) {
  if (threadIdx.x != 0 || S->done) return;
  double T[17];
  for (int k = 0; k < 17; ++k) { double t = 0; for (int w = 0; w < nwg; ++w) t += partial[(size_t)w * 18 + k]; T[k] = t; }
  icp_update(S, T, P);
}

__global__ void __launch_bounds__(ICP_T) icp_fitness(const IcpState* S, const float4* src, const float4* tgt, double* partial) {
  __shared__ float4 s_tile[ICP_TILE];
  __shared__ double s_red[ICP_T / 64][2];
  const int n_src = S->n_src, n_tgt = S->n_tgt;
  const int i = blockIdx.x * ICP_T + threadIdx.x;
  const float4 p0 = src[min(i, n_src - 1)];
  const float* T = S->Tf;
  float4 p;
  p.x = T[0] * p0.x + T[1] * p0.y + T[2] * p0.z + T[3]; p.y = T[4] * p0.x + T[5] * p0.y + T[6] * p0.z + T[7]; p.z = T[8] * p0.x + T[9] * p0.y + T[10] * p0.z + T[11]; p.w = p0.w;
  float d2;
  int idx;
  icp_nn(p, tgt, n_tgt, s_tile, &d2, &idx);
  double s = (i < n_src && idx >= 0) ? (double)d2 : 0.0, c = (i < n_src && idx >= 0) ? 1.0 : 0.0;
  s = bfly_sum_f64(s); c = bfly_sum_f64(c);
  if (lane_id() == 0) { s_red[threadIdx.x >> 6][0] = s; s_red[threadIdx.x >> 6][1] = c; }
  __syncthreads();
  if (threadIdx.x < 2) { double t = 0; for (int w = 0; w < ICP_T / 64; ++w) t += s_red[w][threadIdx.x]; partial[(size_t)blockIdx.x * 18 + threadIdx.x] = t; }
}
__global__ void icp_fitness_final(IcpState* S, const double* partial, int nwg) {
  if (threadIdx.x != 0) return;
  double s = 0, c = 0;
  for (int w = 0; w < nwg; ++w) { s += partial[(size_t)w * 18]; c += partial[(size_t)w * 18 + 1]; }
  S->fitness = c > 0 ? s / c : 1.7976931348623157e308;
}
__global__ void icp_init(IcpState* S, int n_src, const int* n_tgt) {
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 16; ++k) { S->M[k] = (k % 5 == 0) ? 1.f : 0.f; S->Tf[k] = (k % 5 == 0) ? 1.f : 0.f; }
  S->prev_mse = 1.7976931348623157e308; S->fitness = 1.7976931348623157e308;
  S->iter = 0; S->done = (n_src == 0 || *n_tgt == 0) ? 1 : 0; S->converged = 0; S->apply = 0; S->n_src = n_src; S->n_tgt = *n_tgt;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
#include "dev_copy.h"
#include "dev_mem.h"
#include "loop_ctx.h"

int icp_run(const alego_params& P, const alego_kf_in* latest, const alego_kf_in* history, int n_history, alego_icp_result* out,
            alego_point* target_out, int target_cap, hipStream_t st, std::string* err) {
  const int nf = 1 + n_history;
  std::vector<IcpFrame> F(nf);
  std::vector<alego_point> raw;
  int n_src = 0, n_traw = 0;
  for (int f = 0; f < nf; ++f) {
    const alego_kf_in& k = f == 0 ? *latest : history[f - 1];
    if (!kf_in_valid(k)) { *err = "loop closure: null cloud / negative count"; return ALEGO_ERR_ARG; }
    for (int a = 0; a < 6; ++a) F[f].pose[a] = k.pose[a];
    F[f].off[0] = (int)raw.size(); raw.insert(raw.end(), k.corner, k.corner + k.n_corner);
    F[f].off[1] = (int)raw.size(); raw.insert(raw.end(), k.surf, k.surf + k.n_surf);
    F[f].off[2] = (int)raw.size(); raw.insert(raw.end(), k.outlier, k.outlier + k.n_outlier);
    F[f].off[3] = (int)raw.size();
    int& base = f == 0 ? n_src : n_traw;   // destination order: surf, corner, outlier (laserMapping.cpp:794-796,:805-807)
    for (int kind = 0; kind < KF_KINDS; ++kind) F[f].dst[kind] = base + kf_out_start(k.n_corner, k.n_surf, KF_SEL_ALL, kind);
    base += k.n_surf + k.n_corner + k.n_outlier;
  }
  DevPool T;   // temporaries of this call
  IcpFrame* dF; float4 *draw, *dsrc, *dcur, *dtraw, *dtgt; int* dcnt; IcpState* dS; double* dpart;
  const int nwg = std::max(1, (n_src + ICP_T - 1) / ICP_T);
  DevTry c("loop closure", err);
  auto get = [&](auto** p, size_t count) { if (c.ok()) c.took(T.get(p, count, false)); };
  get(&dF, (size_t)nf); get(&draw, raw.size()); get(&dsrc, (size_t)std::max(n_src, 1)); get(&dcur, (size_t)std::max(n_src, 1));
  get(&dtraw, (size_t)std::max(n_traw, 1)); get(&dtgt, (size_t)std::max(n_traw, 1)); get(&dcnt, 2); get(&dS, 1); get(&dpart, (size_t)nwg * 18);
  const int hc[2] = {n_traw, 0};
  if (c.up(dF, F, st).up(draw, raw, st).up(dcnt, hc, st)) return c;
  hipLaunchKernelGGL(icp_build, dim3(8, nf), dim3(ICP_T), 0, st, dF, nf, draw, dsrc, dtraw);
  VoxJob job{dtraw, dcnt, dtgt, dcnt + 1, nullptr, P.lc_leaf, std::max(n_traw, 1), std::max(n_traw, 1), nullptr, 0};
  VoxCtx V;
  if (vox_create(&V, &job, 1, err)) return ALEGO_ERR_HIP;
  int rc = vox_run(V, st, err);
  (void)hipMemcpyAsync(dcur, dsrc, (size_t)n_src * 16, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(icp_init, dim3(1), dim3(64), 0, st, dS, n_src, dcnt + 1);
  const double max_d2 = P.icp_max_corr_dist * P.icp_max_corr_dist;
  for (int it = 0; it < P.icp_max_iters && rc == 0; ++it) {
    hipLaunchKernelGGL(icp_corr, dim3(nwg), dim3(ICP_T), 0, st, dS, dcur, dtgt, max_d2, dpart);
    hipLaunchKernelGGL(icp_step, dim3(1), dim3(64), 0, st, dS, dpart, nwg, P);
  }
  if (n_src > 0) hipLaunchKernelGGL(icp_fitness, dim3(nwg), dim3(ICP_T), 0, st, dS, dsrc, dtgt, dpart);   // (its idle lanes read src[n_src - 1]; without a source the fitness stays icp_init's)
  if (n_src > 0) hipLaunchKernelGGL(icp_fitness_final, dim3(1), dim3(64), 0, st, dS, dpart, nwg);
  IcpState S;
  c.down(&S, dS, 1, st).wait(st);
  if (c.ok() && target_out && S.n_tgt > 0) c.down(target_out, dtgt, (size_t)std::min(S.n_tgt, target_cap));
  vox_destroy(&V);
  if (rc) { *err = "loop closure: VoxelGrid failed"; return ALEGO_ERR_HIP; }
  if (c) return c;
  out->converged = S.converged; out->iterations = S.iter; out->fitness = S.n_src && S.n_tgt ? S.fitness : 1.7976931348623157e308;
  for (int k = 0; k < 16; ++k) out->correction[k] = S.Tf[k];
  out->n_source = S.n_src; out->n_target = S.n_tgt;
  return 0;
}
