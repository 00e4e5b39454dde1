// wave.h — the cross-lane and workgroup primitives every kernel shares: wavefront scans, the workgroup scan, butterfly
// reductions and DPP reductions.  Device functions only; wavefronts of 64 lanes, blockDim.x a multiple of 64.
//
// Names say what a function returns:
//   wave_incl_scan / wave_excl_scan  per-lane prefix sums over the wavefront
//   block_excl_scan<NW>              per-thread prefix sum over a workgroup of NW wavefronts
//   block_min_u64<NW>                the smallest u64 key of a workgroup of NW wavefronts, in every thread
//   bfly_*                           butterfly (__shfl_xor, offsets W/2 -> 1): the result in every lane of each group of W lanes
//   group_*<G>                       DPP inside groups of G consecutive lanes: the result in every lane of the group
//   wave_{min,max,sum}_*             DPP over the wavefront: a uniform value
// The combining order is part of each function's contract (f32 min / max decide the sign of a zero, f64 sums round): a site
// that is compared bit for bit keeps the function it was measured with.
#ifndef ALEGO_WAVE_H_
#define ALEGO_WAVE_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// ---- scans ----
__device__ __forceinline__ int wave_incl_scan(int x) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(x, o, 64); if (lane >= o) x += t; }
  return x;
}
// exclusive prefix; *total = the wavefront's sum (uniform)
__device__ __forceinline__ int wave_excl_scan(int x, int* total) {
  const int incl = wave_incl_scan(x);
  *total = __builtin_amdgcn_readlane(incl, 63);
  return incl - x;
}
// Exclusive prefix of one int per thread over a workgroup of NW wavefronts; *total = the workgroup's sum.  s_w: NW ints of LDS.
// Barriers: one on entry (the previous call's readers of s_w are done), one after the wave totals are written.  None on return:
// s_w is read until the caller's next barrier, so a loop of calls (a chunk carry) needs nothing else.
template <int NW>
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int* total) {
  const int wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v);
  __syncthreads();
  if (lane_id() == 63) s_w[wave] = incl;
  __syncthreads();
  int woff = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) { const int c = s_w[w]; if (w < wave) woff += c; tot += c; }
  *total = tot;
  return woff + incl - v;
}

// ---- butterflies: every lane of a group of W lanes gets the group's value ----
template <int W = 64>
__device__ __forceinline__ int bfly_sum_i32(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W = 64>
__device__ __forceinline__ int bfly_min_i32(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
template <int W = 64>
__device__ __forceinline__ int bfly_max_i32(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
template <int W = 64>
__device__ __forceinline__ unsigned long long bfly_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, o, 64));
  return v;
}
// The smallest of one u64 key per thread over a workgroup of NW wavefronts, in every thread (an arg-min when the key ends in an index;
// a minimum of integers does not depend on the order).  s_min: NW words of LDS.  Barriers: one on entry (the previous call's readers
// of s_min are done), one after the wave minima are written.  None on return: s_min is read until the caller's next barrier, so a
// loop of calls (rounds of "smallest key above the last one") needs nothing else.
template <int NW>
__device__ __forceinline__ unsigned long long block_min_u64(unsigned long long v, unsigned long long* s_min) {
  v = bfly_min_u64(v);
  __syncthreads();
  if (lane_id() == 0) s_min[threadIdx.x >> 6] = v;
  __syncthreads();
  v = s_min[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) v = min(v, s_min[w]);
  return v;
}
// one axis of a bounding box: fminf / fmaxf, min and max interleaved
template <int W = 64>
__device__ __forceinline__ void bfly_minmax_f32(float& mn, float& mx) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
}
__device__ __forceinline__ double bfly_sum_f64(double v) {   // fixed order -> deterministic
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- DPP inside groups of G = 1, 2, 4, 8 or 16 consecutive lanes ----
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror: valid for max / min because they are idempotent
template <int CTRL>
__device__ __forceinline__ int dpp_max_u32_step(int x) {
  const int t = __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, false);
  return (uint32_t)t > (uint32_t)x ? t : x;
}
template <int G>
__device__ __forceinline__ uint32_t group_max_u32(uint32_t v) {
  static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "a DPP group is 1, 2, 4, 8 or 16 lanes");
  int x = (int)v;
  if constexpr (G >= 2) x = dpp_max_u32_step<0xB1>(x);
  if constexpr (G >= 4) x = dpp_max_u32_step<0x4E>(x);
  if constexpr (G >= 8) x = dpp_max_u32_step<0x141>(x);
  if constexpr (G >= 16) x = dpp_max_u32_step<0x140>(x);
  return (uint32_t)x;
}
template <int G>
__device__ __forceinline__ uint32_t group_min_u32(uint32_t v) { return ~group_max_u32<G>(~v); }
// u64: high word first, then the low word among the lanes that hold the winning high word
template <int G>
__device__ __forceinline__ unsigned long long group_min_u64(unsigned long long v) {
  const uint32_t hi = group_min_u32<G>((uint32_t)(v >> 32));
  const uint32_t lo = group_min_u32<G>((uint32_t)(v >> 32) == hi ? (uint32_t)v : 0xFFFFFFFFu);
  return ((unsigned long long)hi << 32) | lo;
}

// ---- DPP over the wavefront: uniform results ----
// max / min of a u32: the 16-lane groups, then the four row results through v_readlane (~12 instructions instead of 6
// dependent ds_bpermute round trips)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  const int x = (int)group_max_u32<16>(v);
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane(x, 0), b = (uint32_t)__builtin_amdgcn_readlane(x, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane(x, 32), e = (uint32_t)__builtin_amdgcn_readlane(x, 48);
  const uint32_t ab = a > b ? a : b, ce = c > e ? c : e;
  return ab > ce ? ab : ce;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  const uint32_t hi = wave_max_u32((uint32_t)(v >> 32));
  const uint32_t lo = wave_max_u32((uint32_t)(v >> 32) == hi ? (uint32_t)v : 0u);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
  const uint32_t hi = wave_min_u32((uint32_t)(v >> 32));
  const uint32_t lo = wave_min_u32((uint32_t)(v >> 32) == hi ? (uint32_t)v : 0xFFFFFFFFu);
  return ((unsigned long long)hi << 32) | lo;
}
// f32 min / max and i32 sum: quad, half row, row, then the row results passed on (row_bcast15, row_bcast31); the value of lane 63
#define ALEGO_DPP_F32(x, ctrl, rmask) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), ctrl, rmask, 0xF, false))
__device__ __forceinline__ float wave_min_f32(float x) {
  x = fminf(x, ALEGO_DPP_F32(x, 0xB1, 0xF)); x = fminf(x, ALEGO_DPP_F32(x, 0x4E, 0xF)); x = fminf(x, ALEGO_DPP_F32(x, 0x141, 0xF)); x = fminf(x, ALEGO_DPP_F32(x, 0x140, 0xF));
  x = fminf(x, ALEGO_DPP_F32(x, 0x142, 0xA)); x = fminf(x, ALEGO_DPP_F32(x, 0x143, 0xC));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ float wave_max_f32(float x) {
  x = fmaxf(x, ALEGO_DPP_F32(x, 0xB1, 0xF)); x = fmaxf(x, ALEGO_DPP_F32(x, 0x4E, 0xF)); x = fmaxf(x, ALEGO_DPP_F32(x, 0x141, 0xF)); x = fmaxf(x, ALEGO_DPP_F32(x, 0x140, 0xF));
  x = fmaxf(x, ALEGO_DPP_F32(x, 0x142, 0xA)); x = fmaxf(x, ALEGO_DPP_F32(x, 0x143, 0xC));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
#undef ALEGO_DPP_F32
__device__ __forceinline__ int wave_sum_i32(int x) {   // (a disabled row keeps `old` = 0: nothing added)
  x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false); x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false); x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false); x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);
  return __builtin_amdgcn_readlane(x, 63);
}

#endif
