// reloc_math.h — the place-recognition rule of alego_loc_relocalize, shared by the kernels (kernels_reloc.hip) and
// the host twins (alego_reloc_descriptor / alego_reloc_match): one definition, so the two cannot drift apart.
//
// DESCRIPTOR of a set of sensor-frame points: RL_NS sectors x RL_NR rings of one byte, sector-major (D[sector][ring], RL_BYTES bytes,
// RL_WORDS words; a sector is RL_SW words).  All arithmetic is f32 without contraction (the build has -ffp-contract=off):
//   a point with a non-finite coordinate is skipped;
//   r = sqrtf((x x) + (y y)), w = (float)max_range / 20.0f, ring = floorf(r / w), skipped unless ring < 20;
//   sector = min(59, floorf((atan2f(y, x) + (float)pi) * (float)(60 / 2 pi))) — atan2f is d_atan2f on the device and libm's on the host,
//   which tests/test_gpu_parity.py pins to each other bit for bit;
//   code = min(255, max(1, floorf((z + z_offset) * 16.0f) + 1));
//   D[sector][ring] = the largest code of its points, 0 when the bin is empty (a maximum of integers does not depend on the order).
// RING KEY: key[ring] = sum over the sectors of D[sector][ring] (at most 60 * 255 = 15300: u16).
// MATCH: dist(Q, M, s) = sum over c, r of |Q[(c + s) mod 60][r] - M[c][r]|; D = min over s, the smallest s attaining it.  Because
// |sum a - sum b| <= sum |a - b|, B = sum over r of |keyQ[r] - keyM[r]| <= dist(Q, M, s) for every s: the bound the search prunes with.
// GUESS: the key pose of the matched frame with yaw - (float)s * (float)(2 pi / 60), f32.
// This rule is the project's own (in the family of Scan Context), chosen so that the device result is exactly defined.
// CANDIDATE WORD: a search result (D, frame id, s) as one u64 whose order by `<` is the order by (D, id, s): D <= 20 * 15300 above bit 32,
// id < 2^24 in bits 8 .. 31, s < 60 in the low byte; RL_CAND_NONE is above every candidate.
// ATTEMPT WINDOW: the history frames an ICP attempt on frame `closest` is aligned to (detectLoopClosure, src/laserMapping.cpp:798-803), for
// alego_loop_search, the appearance search and relocalisation alike.  Plain C++ that a host compiler reads without the HIP runtime.
#ifndef ALEGO_RELOC_MATH_H_
#define ALEGO_RELOC_MATH_H_
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define RL_FN __host__ __device__ inline
#else
#define RL_FN inline
#endif

enum { RL_NS = 60, RL_NR = 20, RL_BYTES = RL_NS * RL_NR, RL_WORDS = RL_BYTES / 4, RL_SW = RL_NR / 4, RL_KEY_WORDS = RL_NR / 2 };
#define RL_DEFAULT_MAX_RANGE 80.0
#define RL_DEFAULT_Z_OFFSET 4.0
#define RL_PI_F 3.14159274101257324f          // (float)pi
#define RL_SECTORS_PER_RAD ((float)(60.0 / (2.0 * 3.14159265358979323846)))
#define RL_RAD_PER_SECTOR ((float)(2.0 * 3.14159265358979323846 / 60.0))

RL_FN float rl_ring_width(double max_range) { return (float)(max_range > 0.0 ? max_range : RL_DEFAULT_MAX_RANGE) / 20.0f; }
RL_FN float rl_z_offset(double z_offset) { return (float)(z_offset - z_offset == 0.0 ? z_offset : RL_DEFAULT_Z_OFFSET); }
RL_FN bool rl_finite(float v) { return v - v == 0.f; }

RL_FN float rl_atan2f(float y, float x) {
#ifdef __HIP_DEVICE_COMPILE__
  return d_atan2f(y, x);   // dev_common.h (included first by the kernels)
#else
  return atan2f(y, x);
#endif
}

// the bin (byte index sector * RL_NR + ring) and code of one point; false: the point is skipped
RL_FN bool rl_bin(float x, float y, float z, float w, float zoff, int* bin, int* code) {
  if (!rl_finite(x) || !rl_finite(y) || !rl_finite(z)) return false;
  const float r = sqrtf((x * x) + (y * y));
  const float fr = floorf(r / w);
  if (!(fr < (float)RL_NR)) return false;
  const float fs = floorf((rl_atan2f(y, x) + RL_PI_F) * RL_SECTORS_PER_RAD);
  const int sector = fs < (float)(RL_NS - 1) ? (int)fs : RL_NS - 1;
  const float fc = fminf(255.f, fmaxf(1.f, floorf((z + zoff) * 16.0f) + 1.f));
  *bin = sector * RL_NR + (int)fr;
  *code = (int)fc;
  return true;
}

RL_FN int rl_abs_diff(int a, int b) { return a > b ? a - b : b - a; }
// B of two ring keys
RL_FN uint32_t rl_key_bound(const uint16_t* kq, const uint16_t* km) {
  uint32_t b = 0;
  for (int r = 0; r < RL_NR; ++r) b += (uint32_t)rl_abs_diff(kq[r], km[r]);
  return b;
}
// f32 yaw of the guess
RL_FN float rl_guess_yaw(float yaw, int shift) { return yaw - (float)shift * RL_RAD_PER_SECTOR; }

// the candidate word
#define RL_CAND_NONE (~0ull)
RL_FN unsigned long long rl_cand_pack(uint32_t dist, uint32_t id, uint32_t shift) { return ((unsigned long long)dist << 32) | ((unsigned long long)id << 8) | shift; }
RL_FN int32_t rl_cand_dist(unsigned long long c) { return (int32_t)(c >> 32); }
RL_FN int32_t rl_cand_id(unsigned long long c) { return (int32_t)((c >> 8) & 0xffffffu); }
RL_FN int32_t rl_cand_shift(unsigned long long c) { return (int32_t)(c & 0xffu); }
// candidate r of a query's row of words -> ids[r], dists[r], shifts[r]; false, and nothing written, when the query has no such candidate
RL_FN bool rl_cand_unpack(const unsigned long long* cand, int r, int32_t* ids, int32_t* dists, int32_t* shifts) {
  if (cand[r] == RL_CAND_NONE) return false;
  ids[r] = rl_cand_id(cand[r]); dists[r] = rl_cand_dist(cand[r]); shifts[r] = rl_cand_shift(cand[r]);
  return true;
}

// the attempt window: frames closest - search_num .. closest + search_num within 0 .. last (the last admissible frame; -1: none, and *jhi < *jlo)
RL_FN void lc_window(int closest, int search_num, int last, int* jlo, int* jhi) {
  *jlo = closest - search_num > 0 ? closest - search_num : 0;
  *jhi = closest + search_num < last ? closest + search_num : last;
}

#endif
