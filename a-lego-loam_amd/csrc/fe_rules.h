// fe_rules.h — the pick rules of feature extraction (src/laserOdometry.cpp:122-293; LO.cpp where alego_params selects its variant): the
// sectors of a ring (:177-181), the curvature sum, its key and thresholds (:122-129,:192,:242), markOccludedPoints (:131-159), the flag byte
// of a point, how far a pick's suppression reaches (:211-234), the label and continuation of a pick by its count (:196-210,:245-251), the tie
// rules of equal curvatures and the membership of less_flat_scan (:279-285).  Three kernel paths pick the same features bit for bit (fe_cand +
// fe_pickc + fe_ring_out; fe_curv + fe_pick4 / fe_pick + fe_voxel + fe_collect); each takes its rules from here.  Plain numbers in, no DevCtx.
// Readable by a host compiler without the HIP runtime: tests/fe_rules/fe_rules_check.cpp checks every rule against the reference's loops
// written out, on the CPU.  Built with -ffp-contract=off everywhere.
#ifndef ALEGO_FE_RULES_H_
#define ALEGO_FE_RULES_H_
#include <stdint.h>

#ifdef __HIPCC__
#define FE_RULE_FN __device__ __forceinline__
FE_RULE_FN uint32_t fe_f32_bits(float f) { return (uint32_t)__float_as_int(f); }
#else
#include <math.h>
#include <string.h>
#define FE_RULE_FN inline
FE_RULE_FN uint32_t fe_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
#endif

// ---- the sectors of a ring [S, E] = [startRingIndex, endRingIndex] (:177-178, LO.cpp:245-249) ----
// first point of sector j; j = n_sectors gives E.  Sectors are contiguous and tile [S, E - 1]: the last point of sector j (:178, :249) is the
// one before the first point of sector j + 1, in both formulas.
FE_RULE_FN int fe_sector_start(int formula, int n_sectors, int S, int E, int j) {
  if (n_sectors == 6) {   // the reference's six sectors: divisions by a constant (a handful of instructions instead of ~35 each)
    if (formula == 0) return (S * (6 - j) + E * j) / 6;
    return S + j * (E - S) / 6;
  }
  if (formula == 0) return (S * (n_sectors - j) + E * j) / n_sectors;
  return S + j * (E - S) / n_sectors;
}
FE_RULE_FN void fe_sector(int formula, int n_sectors, int S, int E, int j, int& sp, int& ep) {
  sp = fe_sector_start(formula, n_sectors, S, E, j); ep = fe_sector_start(formula, n_sectors, S, E, j + 1) - 1;
}
// a sector of fewer than two points is skipped (:181): nothing is picked there and its point is no member of less_flat_scan
FE_RULE_FN bool fe_sector_skipped(int sp, int ep) { return sp >= ep; }
// ... and the skipped sector has a point (an empty one has none): that point is a hole of less_flat_scan
FE_RULE_FN bool fe_sector_lone_point(int sp, int ep) { return fe_sector_skipped(sp, ep) && sp == ep; }

// ---- curvature (:122-129) ----
// points 5 .. M - 6 of the segmented cloud have the eleven taps and take part in markOccludedPoints (:122, :131)
FE_RULE_FN bool fe_has_taps(int i, int M) { return i >= 5 && i < M - 5; }
// the 11-tap sum over the ranges around *r, strictly left to right in f32 (:124)
FE_RULE_FN float fe_curv_sum(const float* r) {
  return r[-5] + r[-4] + r[-3] + r[-2] + r[-1] - r[0] * 10 + r[1] + r[2] + r[3] + r[4] + r[5];
}
// curvature = (double)diff_range * diff_range, exact in fp64 (:125); it orders like |cd|, whose bit pattern orders like an unsigned: the sort key
FE_RULE_FN double fe_curvature(float cd) { const double ad = (double)fabsf(cd); return ad * ad; }
FE_RULE_FN uint32_t fe_curv_key(float cd) { return fe_f32_bits(fabsf(cd)); }
FE_RULE_FN bool fe_curv_edge(double curv, double edge_thres) { return curv > edge_thres; }   // (:192)
FE_RULE_FN bool fe_curv_surf(double curv, double surf_thres) { return curv < surf_thres; }   // (:242)

// ---- markOccludedPoints (:131-159) ----
// per point i, from its ranges r[i - 1], r[i], r[i + 1] and the columns of i and i + 1:
//   A  marks i - 5 .. i and skips the rest (:142-144)     B  marks i + 1 .. i + 5 (:148)     C  parallel beam: marks i (:154-157)
enum { FE_OCCL_A = 1, FE_OCCL_B = 2, FE_OCCL_C = 4 };
FE_RULE_FN int fe_col_dist(int c0, int c1) { const int c = c0 - c1; return c < 0 ? -c : c; }
FE_RULE_FN unsigned fe_occl_marks(int occl_f32, double occl_depth, int occl_col_diff, double parallel_ratio, float r_prev, float r0, float r1, int c0, int c1) {
  bool c1b, c2b;
  double diff1, diff2;
  if (occl_f32) {  // LO.cpp:203-204
    c1b = (double)(r0 - r1) > occl_depth; c2b = (double)(r1 - r0) > occl_depth;
    diff1 = (double)fabsf(r_prev - r0); diff2 = (double)fabsf(r1 - r0);
  } else {         // laserOdometry.cpp:134-135
    const double d1 = (double)r0, d2 = (double)r1;
    c1b = d1 - d2 > occl_depth; c2b = d2 - d1 > occl_depth;
    diff1 = fabs((double)r_prev - d1); diff2 = fabs(d2 - d1);
  }
  const bool near = fe_col_dist(c0, c1) < occl_col_diff;
  const bool A = near && c1b;
  const bool B = near && !c1b && c2b;
  const bool C = !A && diff1 > parallel_ratio * (double)r0 && diff2 > parallel_ratio * (double)r0;
  return (A ? (unsigned)FE_OCCL_A : 0u) | (B ? (unsigned)FE_OCCL_B : 0u) | (C ? (unsigned)FE_OCCL_C : 0u);
}
// the suppression of a pick stops between two points whose columns lie further apart than this (:214, :226)
FE_RULE_FN bool fe_col_jump(int c0, int c1, int suppress_col_diff) { return fe_col_dist(c0, c1) > suppress_col_diff; }

// cloud_neighbor_picked_ of point i after markOccludedPoints: A over [i, i + 5], B over [i - 5, i - 1], C at i.
// Per point: m = the marks of point i, m[-5 .. 5] readable.
FE_RULE_FN bool fe_point_picked(const uint8_t* m) {
  unsigned pk = (m[0] & FE_OCCL_C) ? 1u : 0u;
#pragma unroll
  for (int l = 0; l <= 5; ++l) pk |= (m[l] & FE_OCCL_A);
#pragma unroll
  for (int l = 1; l <= 5; ++l) pk |= (unsigned)(m[-l] & FE_OCCL_B) >> 1;
  return pk != 0;
}
// On lane masks: bit l of a0 / b0 / c0 = the mark of the point in lane l of a 64-point chunk, a1 = the chunk behind it, bp = the chunk in
// front of it; the answer for the point in `lane`.
FE_RULE_FN uint64_t fe_ext128(uint64_t lo, uint64_t hi, int pos) { return (lo >> pos) | (pos ? hi << (64 - pos) : (uint64_t)0); }   // bits [pos, pos + 64) of hi:lo
FE_RULE_FN bool fe_point_picked(uint64_t a0, uint64_t a1, uint64_t bp, uint64_t b0, uint64_t c0, int lane) {
  const bool anyA = (fe_ext128(a0, a1, lane) & 0x3full) != 0;                               // A(i'), i' in [i, i+5]
  const bool anyB = (fe_ext128((bp >> 59) | (b0 << 5), b0 >> 59, lane) & 0x1full) != 0;    // B(i'), i' in [i-5, i-1]
  return ((c0 >> lane) & 1ull) || anyA || anyB;
}

// ---- the flag byte of a point: what the pick kernels of the four-kernel path keep per point ----
enum {
  FE_FLAG_PICKED = 1,        // cloud_neighbor_picked_
  FE_FLAG_GROUND = 2,
  FE_FLAG_EDGE = 4,          // curvature > edge_thres
  FE_FLAG_SURF = 8,          // curvature < surf_thres
  FE_FLAG_LABEL_SHIFT = 4,   // bits 4-5: cloud_label_ + 1 (0 flat, 1 none, 2 less sharp, 3 sharp)
  FE_FLAG_LABEL = 0x30,
  FE_FLAG_JUMP = 64          // fe_col_jump between this point and the next
};
FE_RULE_FN uint8_t fe_flag_of(bool picked, bool ground, bool edge, bool surf, int label, bool jump) {
  return (uint8_t)((picked ? FE_FLAG_PICKED : 0) | (ground ? FE_FLAG_GROUND : 0) | (edge ? FE_FLAG_EDGE : 0) | (surf ? FE_FLAG_SURF : 0) |
                   ((label + 1) << FE_FLAG_LABEL_SHIFT) | (jump ? FE_FLAG_JUMP : 0));
}
FE_RULE_FN int fe_flag_label(unsigned flag) { return (int)((flag >> FE_FLAG_LABEL_SHIFT) & 3u) - 1; }
FE_RULE_FN uint8_t fe_flag_with_label(unsigned flag, int label) { return (uint8_t)((flag & ~(unsigned)FE_FLAG_LABEL) | ((unsigned)(label + 1) << FE_FLAG_LABEL_SHIFT)); }
// not picked, not ground, curvature > edge_thres (:190-192) / not picked, ground, curvature < surf_thres (:240-242)
FE_RULE_FN bool fe_sharp_candidate(bool picked, bool ground, bool edge) { return !picked && !ground && edge; }
FE_RULE_FN bool fe_flat_candidate(bool picked, bool ground, bool surf) { return !picked && ground && surf; }
FE_RULE_FN bool fe_sharp_candidate(int flag) { return (flag & (FE_FLAG_PICKED | FE_FLAG_GROUND | FE_FLAG_EDGE)) == FE_FLAG_EDGE; }
FE_RULE_FN bool fe_flat_candidate(int flag) { return (flag & (FE_FLAG_PICKED | FE_FLAG_GROUND | FE_FLAG_SURF)) == (FE_FLAG_GROUND | FE_FLAG_SURF); }
// less_flat_scan holds the points of the picked sectors with cloud_label_ <= 0 (:279-285)
FE_RULE_FN constexpr bool fe_less_flat_member(int label) { return label <= 0; }

// ---- how far the suppression of a pick at c reaches (:211-234): up to suppress_radius (<= 5) points either way, stopping at the first jump ----
// jumps_fwd bit l = fe_col_jump between c + l and c + l + 1; jumps_bwd bit l = between c - l - 1 and c - l (bit 0 next to the pick either way)
struct FeReach { int fwd, bwd; };
FE_RULE_FN int fe_reach_one(unsigned jumps, int suppress_radius) {
  const int first = __builtin_ctz((jumps & 0x1fu) | 0x20u);
  return first < suppress_radius ? first : suppress_radius;
}
FE_RULE_FN FeReach fe_reach(unsigned jumps_fwd, unsigned jumps_bwd, int suppress_radius) {
  FeReach r;
  r.fwd = fe_reach_one(jumps_fwd, suppress_radius); r.bwd = fe_reach_one(jumps_bwd, suppress_radius);
  return r;
}
// the same from a window of jump bits in point order: jumps_before bit 4 = the jump between c - 1 and c, bit 0 = between c - 5 and c - 4
FE_RULE_FN int fe_reach_bwd_window(unsigned jumps_before, int suppress_radius) {
  const int first = __builtin_clz(((jumps_before & 0x1fu) << 27) | 0x04000000u);
  return first < suppress_radius ? first : suppress_radius;
}

// ---- label / continuation of the pick that has just been counted (:196-210, :245-251); picked = its number in the sector, from 1 ----
//   lab     2 sharp, 1 less sharp, 0 none (the (n_less_sharp + 1)-th: marked picked, not labelled, not spread, ends the loop :207-210), -1 flat
//   spread  the pick suppresses its neighbours (the n_flat-th flat pick ends the loop before the suppression, :248-251)
//   more    the loop goes on; nmax: a path that leaves the unlabelled last sharp pick out (it changes no output) passes max(n_sharp, n_less_sharp),
//           one that takes it INT_MAX
template <bool FLAT>
FE_RULE_FN void fe_pick_label(int n_sharp, int n_less_sharp, int n_flat, int picked, int nmax, int& lab, bool& spread, bool& more) {
  if (FLAT) { lab = -1; more = picked < n_flat; spread = more; }
  else { lab = picked <= n_sharp ? 2 : (picked <= n_less_sharp ? 1 : 0); spread = lab != 0; more = lab != 0 && picked < nmax; }
}

// ---- the order of the picks: the reference sorts a sector by curvature and scans it descending (sharp) / ascending (flat) ----
// A pick is the best remaining candidate.  Candidates looked at in ascending index order: does one with key k replace the best so far, b?
// Equal curvatures: sharp takes the larger index (the scan runs from the sorted sector's end), flat the smaller.
template <bool FLAT> FE_RULE_FN constexpr uint32_t fe_key_none() { return FLAT ? 0xFFFFFFFFu : 0u; }   // no candidate: what every real key beats
template <bool FLAT> FE_RULE_FN bool fe_scan_takes(uint32_t k, uint32_t b) { return FLAT ? k < b : k >= b; }
// (fe_tie_takes / fe_tie_takes_arranged are the specification: the kernels decide a tie by a max (sharp) / min (flat) reduction over the tied candidates'
// indices or fe_arranged_code, which takes the same candidate; the host test holds the reductions' order against these two)
template <bool FLAT> FE_RULE_FN bool fe_tie_takes(int idx, int idx_best) { return FLAT ? idx < idx_best : idx > idx_best; }
// sort_mode 2: equal curvatures in the order libstdc++'s std::sort leaves them in (stdsort_emu.h): sharp takes the later position of that
// arrangement, flat the earlier.  As one code per candidate, `local` = its index in the sector (< 65536): the pick is the largest code (sharp) /
// the smallest (flat), and 0 / 0xFFFFFFFF is no candidate's.
template <bool FLAT> FE_RULE_FN bool fe_tie_takes_arranged(int pos, int pos_best) { return FLAT ? pos < pos_best : pos > pos_best; }
template <bool FLAT> FE_RULE_FN uint32_t fe_arranged_code(uint32_t pos, uint32_t local) { return ((pos + (FLAT ? 0u : 1u)) << 16) | local; }

#endif
