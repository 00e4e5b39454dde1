// dev_cost.h — the device side of the solvers' evaluations: the rotation helpers beyond solve_rows.h (the cost functors and the trust-region
// control, host-compilable), the cooperative pose terms and the workgroup reductions of the normal equations.
#ifndef ALEGO_DEV_COST_H_
#define ALEGO_DEV_COST_H_

#include "dev_common.h"
#include <type_traits>
#include "solve_rows.h"

DEV_INLINE void dq_to_mat(const DQuat& q, double R[9]) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
DEV_INLINE DQuat dq_from_mat(const double m[9]) {
  DQuat q;
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0); q.w = 0.5 * t; t = 0.5 / t;
    q.x = (m[7] - m[5]) * t; q.y = (m[2] - m[6]) * t; q.z = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
    double v[3];
    v[i] = 0.5 * t; t = 0.5 / t;
    q.w = (m[k * 3 + j] - m[j * 3 + k]) * t;
    v[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
    v[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    q.x = v[0]; q.y = v[1]; q.z = v[2];
  }
  return q;
}
// dq_from_mat with the largest-diagonal branch spelt out per axis: the same operations in the same order, without the dynamically indexed
// locals that put a small kernel's frame in scratch (rl_apply, kernels_reloc.hip); test_relocalize.py pins the two to each other bit for bit
template <int I> DEV_INLINE DQuat dq_from_mat_diag(const double* m) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double t = sqrt(m[I * 3 + I] - m[J * 3 + J] - m[K * 3 + K] + 1.0);
  double v[3];
  v[I] = 0.5 * t; t = 0.5 / t;
  DQuat q;
  q.w = (m[K * 3 + J] - m[J * 3 + K]) * t;
  v[J] = (m[J * 3 + I] + m[I * 3 + J]) * t;
  v[K] = (m[K * 3 + I] + m[I * 3 + K]) * t;
  q.x = v[0]; q.y = v[1]; q.z = v[2];
  return q;
}
DEV_INLINE DQuat dq_from_mat_flat(const double* m) {
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    DQuat q;
    t = sqrt(t + 1.0); q.w = 0.5 * t; t = 0.5 / t;
    q.x = (m[7] - m[5]) * t; q.y = (m[2] - m[6]) * t; q.z = (m[3] - m[1]) * t;
    return q;
  }
  if (m[4] > m[0]) return m[8] > m[4] ? dq_from_mat_diag<2>(m) : dq_from_mat_diag<1>(m);
  return m[8] > m[0] ? dq_from_mat_diag<2>(m) : dq_from_mat_diag<0>(m);
}
DEV_INLINE DQuat dq_inverse(const DQuat& q) {
  const double n2 = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
  return DQuat{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
}
DEV_INLINE DQuat ldq(const double* p) { return DQuat{p[0], p[1], p[2], p[3]}; }
DEV_INLINE void stq(double* p, const DQuat& q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }
// correctPoses (laserMapping.cpp:579-580): the pose (q[4], t[3]) <- [R | c] * pose, rc_ the 3x4 [R | c] of a loop-closure correction (f32 or f64)
// (FLAT: dq_from_mat_flat instead of dq_from_mat, for kernels that must stay out of scratch)
template <class T, bool FLAT = false> DEV_INLINE void dq_apply_correction(double* q, double* t3, const T* rc_) {
  double rc[12], R[9], M[9], t[3];
  for (int k = 0; k < 12; ++k) rc[k] = (double)rc_[k];
  dq_to_mat(ldq(q), R);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[i * 3 + j] = rc[i * 4 + 0] * R[0 * 3 + j] + rc[i * 4 + 1] * R[1 * 3 + j] + rc[i * 4 + 2] * R[2 * 3 + j];
  for (int i = 0; i < 3; ++i) t[i] = rc[i * 4 + 0] * t3[0] + rc[i * 4 + 1] * t3[1] + rc[i * 4 + 2] * t3[2] + rc[i * 4 + 3];
  if constexpr (FLAT) stq(q, dq_from_mat_flat(M)); else stq(q, dq_from_mat(M));
  for (int i = 0; i < 3; ++i) t3[i] = t[i];
}

// The same terms computed cooperatively by a workgroup: six lanes take one angle each (the three half angles of the
// quaternion, the three full angles of the Jacobian terms), everybody assembles the result from LDS.  Evaluating the
// nine sin/cos pairs in every thread cost ~2000 fp64 instructions per wavefront and solver evaluation — most of what
// lo_solve / lm_solve issued.  Same sin()/cos() calls on the same arguments: bit-identical to pose_terms().
// Ends with a barrier; the caller must pass another barrier before the next call (block_reduce28 does).
DEV_INLINE PoseTerms pose_terms_coop(const double* p, double* s_trig /*[12] LDS*/) {
  const int tid = threadIdx.x;
  if (tid < 6) {
    const double a = tid == 0 ? 0.5 * p[5] : tid == 1 ? 0.5 * p[4] : tid == 2 ? 0.5 * p[3] : tid == 3 ? p[3] : tid == 4 ? p[4] : p[5];
    s_trig[2 * tid] = cos(a);
    s_trig[2 * tid + 1] = sin(a);
  }
  __syncthreads();
  PoseTerms T;
  const DQuat qz{s_trig[0], 0, 0, s_trig[1]}, qy{s_trig[2], 0, s_trig[3], 0}, qx{s_trig[4], s_trig[5], 0, 0};
  T.q = dq_mul(dq_mul(qz, qy), qx);
  T.t[0] = p[0]; T.t[1] = p[1]; T.t[2] = p[2];
  T.cr = s_trig[6]; T.sr = s_trig[7]; T.cp = s_trig[8]; T.sp = s_trig[9]; T.cy = s_trig[10]; T.sy = s_trig[11];
  return T;
}

// Deterministic workgroup reduction of the 28 normal-equation scalars.  Each quad of lanes first adds its four
// partials with two DPP quad_perm steps (no LDS), one lane per quad stores the sums k-major (conflict-free),
// then a group of lanes per scalar finishes (below).  The quad step keeps the LDS footprint at 28 x T/4 doubles
// (28 KB for 512 threads): these solver workgroups live for hundreds of microseconds, and their LDS is what keeps other
// streams' workgroups off the CU.  (An earlier version let 4 threads per scalar add 32 entries each and a third stage add
// the 4 sums: 30 % of lm_solve's time.)
template <int CTRL>
DEV_INLINE double dpp_add_f64(double v) {   // v + (v of the lane selected by the DPP control CTRL)
  const long long b = __double_as_longlong(v);
  const int lo = (int)(unsigned)(unsigned long long)b, hi = (int)(unsigned)((unsigned long long)b >> 32);
  const int plo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false), phi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return v + __longlong_as_double((long long)(((unsigned long long)(unsigned)phi << 32) | (unsigned)plo));
}
// PRE DPP steps come before LDS: 2 (the quad step above, 64 .. 512 threads) or 3 (a row_half_mirror step more: 14 KB for 512 threads; 128 .. 1024
// threads — lm_solve keeps its residual rows in LDS, so every KB of reduction scratch is 20 rows streamed from the L2 instead).  Q = T >> PRE partials
// per scalar; G = Q/8 lanes per scalar (16 ... 2) add 8 strided partials each and finish with log2(G) DPP steps inside their row: two barriers.
template <int PRE>
DEV_INLINE double block_reduce_head(double v) {
  static_assert(PRE == 2 || PRE == 3, "a quad or eight lanes before LDS");
  v = dpp_add_f64<0xB1>(v);                 // lane ^ 1: both lanes of a pair hold a + b (commutative: identical bits)
  v = dpp_add_f64<0x4E>(v);                 // lane ^ 2: all four lanes hold (a + b) + (c + d)
  if (PRE == 3) v = dpp_add_f64<0x141>(v);  // row_half_mirror: all eight lanes hold ((a + b) + (c + d)) + ((e + f) + (g + h))
  return v;
}
template <int G>
DEV_INLINE double block_reduce_tail(const double* s /* partials of one scalar, + the lane's index in its group */) {
  static_assert(G == 2 || G == 4 || G == 8 || G == 16, "8 partials per lane, 2 .. 16 lanes per scalar");
  double t = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) t += s[j * G];
  t = dpp_add_f64<0xB1>(t);
  if (G >= 4) t = dpp_add_f64<0x4E>(t);
  if (G >= 8) t = dpp_add_f64<0x141>(t);   // row_half_mirror: the two quads of an 8-lane group
  if (G == 16) t = dpp_add_f64<0x140>(t);  // row_mirror: the two halves of a row
  return t;
}
template <int T, int PRE>
DEV_INLINE void block_reduce28(const double acc[28], double* s_acc /*[28 * (T >> PRE)]*/, double* s_out /*[28]*/) {
  constexpr int Q = T >> PRE, G = Q / 8;
  static_assert(28 * G <= T, "one lane group per scalar");
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 28; ++k) {
    const double v = block_reduce_head<PRE>(acc[k]);
    if ((tid & ((1 << PRE) - 1)) == 0) s_acc[k * Q + (tid >> PRE)] = v;
  }
  __syncthreads();
  if (tid < 28 * G) {   // whole lane groups: the DPP steps of the tail never leave a group
    const int k = tid / G, g = tid - k * G;
    const double t = block_reduce_tail<G>(s_acc + k * Q + g);
    if (g == 0) s_out[k] = t;
  }
  __syncthreads();
}
// The reduction tree of scalar 27 (the cost) on its own: the same DPP steps, the same eight strided LDS partials per lane of a group of G, the
// same DPP finish — s_out[27] is the double block_reduce28 delivers for the same per-thread partials (lanes [0, G) stand in for lanes
// [27 G, 28 G): both groups start at a multiple of G, so every DPP step pairs the same partials).
template <int T, int PRE>
DEV_INLINE void block_reduce_cost(double cost, double* s_acc /*[T >> PRE]*/, double* s_out /*[28]*/) {
  constexpr int G = (T >> PRE) / 8;
  const int tid = threadIdx.x;
  const double v = block_reduce_head<PRE>(cost);
  if ((tid & ((1 << PRE) - 1)) == 0) s_acc[tid >> PRE] = v;
  __syncthreads();
  if (tid < G) {
    const double t = block_reduce_tail<G>(s_acc + tid);
    if (tid == 0) s_out[27] = t;
  }
  __syncthreads();
}

// ---- one evaluation and one solve by a workgroup of T threads (lo_solve_t, lm_solve, lm_shard_eval, lm_regcov) ----
// The phases a -DALEGO_TIMING build clocks, in ticks per thread: lo_times[k] (wall clock) and lm_solve's ld[43 + k]; empty in the default build
enum { WG_T_POSE = 0, WG_T_ROWS, WG_T_REDUCE, WG_T_CONTROL, WG_T_COUNT = 6 };
template <bool WALL> struct WgClock {
#ifdef ALEGO_TIMING
  long long tm[WG_T_COUNT] = {0, 0, 0, 0, 0, 0}, t0 = 0;
  DEV_INLINE static long long now() { return WALL ? (long long)wall_clock64() : (long long)clock64(); }
  DEV_INLINE void begin() { t0 = now(); }
  DEV_INLINE void end(int k) { tm[k] += now() - t0; }
#else
  DEV_INLINE void begin() {}
  DEV_INLINE void end(int) {}
#endif
};

// x -> s_out[28] (FULL) or s_out[27] alone: the pose terms, then rows(T, acc, std::bool_constant<FULL>) sums this thread's rows, then the reduction
template <int T, int PRE, bool FULL, class Rows, class Clock>
DEV_INLINE void wg_evaluate(const double* x, double* s_trig /*[12]*/, double* s_acc, double* s_out, Rows&& rows, Clock& ck) {
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0;
  ck.begin();
  const PoseTerms P = pose_terms_coop(x, s_trig);
  ck.end(WG_T_POSE);
  ck.begin();
  rows(P, acc, std::bool_constant<FULL>{});
  ck.end(WG_T_ROWS);
  ck.begin();
  if constexpr (FULL) block_reduce28<T, PRE>(acc, s_acc, s_out); else block_reduce_cost<T, PRE>(acc[27], s_acc, s_out);
  ck.end(WG_T_REDUCE);
}

// One ceres::Solve into S: evaluate what `kind` asks for, let thread 0 take the sums in and propose (lm_control), until the solve has ended.
// kind: LM_EV_BEGIN (from x0) or LM_EV_AGAIN (from S.x, whose normal equations S still holds: no evaluation; LaserMapping alone enters it).
// Hook (lm_solve_remap alone; WgNoHook: nothing, the solve as it always was): after_begin(x0, s_trig, s_out) is called by every thread between the
// evaluation of LM_EV_BEGIN and the control thread's turn — behind the barrier that published s_out, s_trig still holding pose_terms_coop's sines and
// cosines of x0, and thread 0 runs it before lm_control; proj()
// is what that thread hands lm_step (solve_rows.h).
struct WgNoHook {
  static constexpr bool remap = false;
  DEV_INLINE void after_begin(const double*, const double*, const double*) const {}
  DEV_INLINE const double* proj() const { return nullptr; }
};
template <int T, int PRE, bool FULL_EVAL, class Rows, class Clock, class Hook = WgNoHook>
DEV_INLINE void wg_solve(LmState& S, int* s_action, int kind, const double* x0, int max_iter, double* s_trig, double* s_acc, double* s_out, Rows&& rows, Clock& ck,
                         const Hook& hook = Hook{}) {
  while (true) {
    double x[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = kind == LM_EV_BEGIN ? x0[k] : kind == LM_EV_JAC ? S.x[k] : kind == LM_EV_AGAIN ? 0.0 : S.cand[k];
    if (kind == LM_EV_CAND_COST) wg_evaluate<T, PRE, false>(x, s_trig, s_acc, s_out, rows, ck);
    else if (kind != LM_EV_AGAIN) wg_evaluate<T, PRE, true>(x, s_trig, s_acc, s_out, rows, ck);
    ck.begin();
    if constexpr (Hook::remap) hook.after_begin(x0, s_trig, s_out);
    if (threadIdx.x == 0) *s_action = lm_control<FULL_EVAL, ALEGO_SOLVE_SPECULATE != 0, Hook::remap>(S, kind, x0, s_out, max_iter, hook.proj());
    __syncthreads();
    ck.end(WG_T_CONTROL);
    const int act = *s_action;
    if (act == LM_STOP) break;
    kind = lm_next_eval<FULL_EVAL>(act);   // (an evaluation and its barriers lie between this read of s_action and the next write)
  }
}

#endif
