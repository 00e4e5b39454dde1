// kernels_edt.hip — the exact squared Euclidean distance transform of the classified occupancy grid and the inflated cost map on gfx950
// (alego_occ_distance, alego_occ_costmap).  The rule is edt_math.h's; the host (lm_host.hip) classifies into the class
// array first and owns every buffer.
//
//   edt_pass_x    one wavefront per (y, z) line, 64 cells of x per step.  Going down the line the wavefront keeps each block's ballot of
//                 sources and the first source beyond the block in LDS; going up, a lane finds its nearest source to the left from the
//                 block's ballot below its own bit (else the last source of the blocks before, a running scalar) and to the right from the
//                 ballot above it (else the block's LDS word).  The classes are read once and g^2 written once, both contiguous.
//   edt_pass_y,   passes Y and Z (one body, edt_env_line; two names so that a profile tells them apart): one lane per line, adjacent lanes
//   edt_pass_z    at adjacent x, so every step of the wavefront touches 64 consecutive cells and nothing is transposed.  edt_envelope's
//                 stack lives in device memory as int2 (cell | start << 16, f), entry q of line l at env[q lines + l]: the 64 lanes'
//                 entries of one depth are consecutive.  The two upper entries of the stack and the values of the next cells are in
//                 registers.
//   edt_finish    the cap, and the three statistics by wavefront reductions, LDS and one atomic per workgroup and counter.
//   edt_cost_k    edt_cost per cell over the classes, d2 and the table.
// Every index formed from n[] is tested against its array's size before it is followed; all stores are plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/alego_mi355x.h"
#include "edt_math.h"
#include "occ.h"
#include "prof.h"
#include "wave.h"

#define EDT_T 256      // edt_pass_x: four lines per workgroup; edt_finish, edt_cost_k
#define EDT_ENV_T 64   // edt_pass_y / _z: one wavefront of lines per workgroup, so that few lines still spread over the CUs

__global__ void __launch_bounds__(EDT_T) edt_pass_x(const int8_t* __restrict__ cls, int n0, long long lines, size_t cells, int unknown_is_obstacle,
                                                    uint32_t* __restrict__ out) {
  extern __shared__ unsigned long long edt_smem[];   // [EDT_T / 64][nb] ballots, then [EDT_T / 64][nb] ints: the first source beyond the block
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int nb = (n0 + 63) >> 6;
  unsigned long long* s_mask = edt_smem + (size_t)wave * nb;
  int* s_next = reinterpret_cast<int*>(edt_smem + (size_t)(EDT_T / 64) * nb) + (size_t)wave * nb;
  const long long line = (long long)blockIdx.x * (EDT_T / 64) + wave;
  const bool live = line < lines;
  const size_t base = live ? (size_t)line * n0 : 0;
  int next = n0;
  for (int b = nb - 1; b >= 0; --b) {
    const int x = b * 64 + lane;
    bool src = false;
    if (live && x < n0 && base + x < cells) src = edt_source(cls[base + x], unknown_is_obstacle);
    const unsigned long long m = __ballot(src);
    if (lane == 0) { s_mask[b] = m; s_next[b] = next; }
    if (m) next = b * 64 + __ffsll(m) - 1;
  }
  __syncthreads();   // (every wavefront of the workgroup makes the same nb steps)
  int last = -1;
  for (int b = 0; b < nb; ++b) {
    const unsigned long long m = s_mask[b];
    const int x = b * 64 + lane;
    const unsigned long long below = m & ((2ull << lane) - 1ull), above = m >> lane;   // the lane's own bit is in both
    const int left = below ? b * 64 + 63 - __clzll((long long)below) : last;
    const int right = above ? x + __ffsll(above) - 1 : s_next[b];
    if (live && x < n0 && base + x < cells) out[base + x] = edt_g2(x, left, right, n0);
    if (m) last = b * 64 + 63 - __clzll((long long)m);
  }
}

namespace {
struct EdtLoad {
  const uint32_t* p; size_t base, stride, cells;
  __host__ __device__ uint32_t operator()(int32_t u) const { const size_t i = base + (size_t)u * stride; return (u >= 0 && i < cells) ? p[i] : EDT_FAR; }
};
struct EdtStore {
  uint32_t* p; size_t base, stride, cells;
  __host__ __device__ void operator()(int32_t u, int64_t v) const { const size_t i = base + (size_t)u * stride; if (i < cells) p[i] = v < 0 ? EDT_FAR : (uint32_t)v; }
};
struct EdtStack {   // an entry: (cell | start << 16, f); both are below 65536 (edt_dims_fault)
  int2* e; size_t line, lines, cap;
  __host__ __device__ void put(int32_t q, const EdtTop& v) const {
    const size_t i = (size_t)q * lines + line;
    if (q >= 0 && i < cap) e[i] = make_int2((int)((uint32_t)v.i | ((uint32_t)v.t << 16)), (int)v.f);
  }
  __host__ __device__ EdtTop get(int32_t q) const {
    const size_t i = (size_t)q * lines + line;
    const int2 v = (q >= 0 && i < cap) ? e[i] : make_int2(0, 0);
    return EdtTop{(int32_t)((uint32_t)v.x & 0xFFFFu), (int32_t)((uint32_t)v.x >> 16), (uint32_t)v.y};
  }
};
}  // namespace

// lines of `len` cells at stride `inner`: line l starts at (l / inner) len inner + l % inner (pass Y: inner = n0; pass Z: inner = n0 n1)
__device__ __forceinline__ void edt_env_line(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int2* __restrict__ env, size_t env_cap, int len, long long inner,
                                             long long lines, size_t cells) {
  const long long l = (long long)blockIdx.x * EDT_ENV_T + threadIdx.x;
  if (l >= lines) return;
  const size_t base = (size_t)(l / inner) * ((size_t)len * (size_t)inner) + (size_t)(l % inner);
  edt_envelope(len, EdtLoad{in, base, (size_t)inner, cells}, EdtStore{out, base, (size_t)inner, cells}, EdtStack{env, (size_t)l, (size_t)lines, env_cap}, EdtNoCheck());
}
__global__ void __launch_bounds__(EDT_ENV_T) edt_pass_y(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int2* __restrict__ env, size_t env_cap, int len,
                                                        long long inner, long long lines, size_t cells) {
  edt_env_line(in, out, env, env_cap, len, inner, lines, cells);
}
__global__ void __launch_bounds__(EDT_ENV_T) edt_pass_z(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int2* __restrict__ env, size_t env_cap, int len,
                                                        long long inner, long long lines, size_t cells) {
  edt_env_line(in, out, env, env_cap, len, inner, lines, cells);
}

// stats: sources, FAR cells, the largest finite d2 + 1 (0: none); zeroed by the launch.  The wavefronts' counts meet in LDS: three atomics per workgroup.
__global__ void __launch_bounds__(EDT_T) edt_finish(uint32_t* __restrict__ d2, size_t cells, uint32_t r2, unsigned long long* __restrict__ stats) {
  __shared__ unsigned s_cnt[2], s_max;
  if (threadIdx.x == 0) { s_cnt[0] = 0; s_cnt[1] = 0; s_max = 0; }
  __syncthreads();
  int sources = 0, far = 0;
  uint32_t mx = 0;
  for (size_t i = (size_t)blockIdx.x * EDT_T + threadIdx.x; i < cells; i += (size_t)gridDim.x * EDT_T) {
    const uint32_t raw = d2[i], v = edt_cap(raw, r2);
    if (v != raw) d2[i] = v;
    sources += v == 0;
    if (v == EDT_FAR) ++far; else if (v + 1 > mx) mx = v + 1;
  }
  sources = wave_sum_i32(sources); far = wave_sum_i32(far); mx = wave_max_u32(mx);
  if (lane_id() == 0) {
    if (sources) atomicAdd(&s_cnt[0], (unsigned)sources);
    if (far) atomicAdd(&s_cnt[1], (unsigned)far);
    if (mx) atomicMax(&s_max, mx);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(stats + ALEGO_EDT_SOURCES, (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(stats + ALEGO_EDT_FAR_CELLS, (unsigned long long)s_cnt[1]);
    if (s_max) atomicMax(stats + ALEGO_EDT_MAX_D2, (unsigned long long)s_max);
  }
}

__global__ void __launch_bounds__(EDT_T) edt_cost_k(const int8_t* __restrict__ cls, const uint32_t* __restrict__ d2, size_t cells, int unknown_is_obstacle,
                                                    const uint8_t* __restrict__ table, int n_table, int inflate_unknown, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * EDT_T + threadIdx.x; i < cells; i += (size_t)gridDim.x * EDT_T)
    out[i] = edt_cost(cls[i], d2[i], unknown_is_obstacle, table, n_table, inflate_unknown);
}

uint32_t* launch_edt(const EdtWork& W, hipStream_t st) {
  const long long n0 = W.n[0], n1 = W.n[1], n2 = W.n[2];
  const size_t cells = (size_t)(n0 * n1 * n2);
  uint32_t *in = W.a, *out = W.b;
  {
    const long long lines = n1 * n2;
    const int nb = (int)((n0 + 63) >> 6);
    ALEGO_LAUNCH(edt_pass_x, dim3((unsigned)((lines + EDT_T / 64 - 1) / (EDT_T / 64))), dim3(EDT_T), (size_t)(EDT_T / 64) * nb * 12, st, W.cls, (int)n0, lines, cells,
                 W.unknown_is_obstacle, in);
  }
  for (int axis = 1; axis <= 2; ++axis) {
    const long long len = W.n[axis], inner = axis == 1 ? n0 : n0 * n1, lines = (long long)cells / len;
    if (len <= 1) continue;
    const dim3 grid((unsigned)((lines + EDT_ENV_T - 1) / EDT_ENV_T));
    if (axis == 1) ALEGO_LAUNCH(edt_pass_y, grid, dim3(EDT_ENV_T), 0, st, in, out, W.env, W.env_cap, (int)len, inner, lines, cells);
    else ALEGO_LAUNCH(edt_pass_z, grid, dim3(EDT_ENV_T), 0, st, in, out, W.env, W.env_cap, (int)len, inner, lines, cells);
    std::swap(in, out);
  }
  (void)hipMemsetAsync(W.stats, 0, ALEGO_EDT_STATS * sizeof(unsigned long long), st);
  const int nbk = (int)std::min<size_t>((cells + 8 * EDT_T - 1) / (8 * EDT_T), 2048);   // eight cells per thread or more: few atomics
  ALEGO_LAUNCH(edt_finish, dim3(nbk), dim3(EDT_T), 0, st, in, cells, W.r2, W.stats);
  return in;
}

void launch_edt_cost(const int8_t* cls, const uint32_t* d2, size_t cells, int unknown_is_obstacle, const uint8_t* table, int n_table, int inflate_unknown, uint8_t* out,
                     hipStream_t st) {
  const int nb = (int)std::min<size_t>((cells + EDT_T - 1) / EDT_T, 65536);
  ALEGO_LAUNCH(edt_cost_k, dim3(nb), dim3(EDT_T), 0, st, cls, d2, cells, unknown_is_obstacle, table, n_table, inflate_unknown, out);
}
