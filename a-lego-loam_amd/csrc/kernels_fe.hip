// kernels_fe.hip — feature extraction on gfx950 (replaces src/laserOdometry.cpp:122-293).
//
//   fe_curv    a7,a8: 11-tap f32 curvature sum through an LDS window + occlusion / parallel-beam
//              marking written as a gather (no atomics) (:122-159), and the flag byte of every point for the pick
//   fe_pick4   a9: four rings per wavefront (one 16-lane DPP row each); the reference's "sort, then scan
//              descending/ascending" is evaluated as repeated row-wide arg-max / arg-min over the
//              not-yet-picked candidates of the sector (identical result for the total order
//              (curvature, index)); +-5 neighbour suppression by ballot         (:172-286)
//   fe_pick    the same with one ring per wavefront (ALEGO_FE_PICK1, very long sectors)
//   fe_voxel   a10: per-ring pcl::VoxelGrid(0.4): runs of consecutive equal voxel ids ordered through
//              monotone buckets in LDS, centroid in sorted (= original) order    (:288-293)
//   fe_collect ring-ascending concatenation into the four feature clouds (:199-205,:245,:293) + bounding boxes of 32 consecutive
//              less_flat / less_sharp points for the next scan's LaserOdometry
//
// Where the rules live.  fe_rules.h (host-readable, pinned by tests/test_fe_rules.py): the sectors of a ring and which are skipped, the
// curvature sum / key / thresholds, the occlusion marks and "a point is picked", the flag byte and its candidate tests, the suppression
// reach, label / spread / continuation of a pick by its count, the tie rules (by index; by std::sort's arrangement under sort_mode 2),
// less_flat_scan membership.  fe_common.h (device): fe_curv's body, the concatenation of the pick clouds with the less_sharp boxes
// (fe_concat_picks / fe_concat_cloud, shared with fe_ring_out's row NS), the bucket tables of the run ordering (fe_buckets*, shared with
// fe_ring_out).  This file keeps what is a kernel's own: who owns which sector element, the reductions, the LDS updates.
#include <cstdlib>
#include <type_traits>
#include "dev_common.h"
#include "fe_common.h"
#include "front_end.h"
#include "prof.h"
#include "stdsort_emu.h"
#include "vgrid.h"

#define FE_BLOCK 256
#define FE_CW 1024   // points per fe_curv workgroup
#define FE_MAXH 4096  // largest horizon_scan supported by the per-ring LDS staging
// fe_pick<FE_T>: sector elements per lane kept in registers (sector length <= 64*FE_T): 6 covers 16x1800
// (<= 300 points per sector), 12 covers horizon_scan 4096 (683)

__global__ void __launch_bounds__(FE_BLOCK) fe_curv(DevCtx d) {
  const int slot = blockIdx.y + d.slot0;
  const int M = scal_of(d, slot)[SC_M];
  const int t0 = blockIdx.x * FE_CW;   // FE_CW points per workgroup, FE_CW / FE_BLOCK per thread
  if (t0 >= M) return;
  __shared__ float s_r[FE_CW + 2 * FE_HALO];
  __shared__ int s_c[FE_CW + 2 * FE_HALO];
  __shared__ uint8_t s_f[FE_CW + 2 * FE_HALO];
  fe_curv_chunk<FE_BLOCK, FE_CW>(d, slot, M, t0, s_r, s_c, s_f);
}

// The greedy pick of fe_pick and fe_pick4 (:189-277).  The reference's "sort, then scan descending / ascending" only ever asks for the best remaining
// candidate of the sector; the kernels below find it by repeated arg-max (sharp / less sharp) or arg-min (flat) over the curvature keys, one loop
// templated on FLAT.  What is best, who wins a tie, what label a pick gets, whether it spreads and whether the loop goes on: fe_rules.h.
template <bool FLAT> DEV_INLINE uint32_t fe_better(uint32_t a, uint32_t b) { return FLAT ? min(a, b) : max(a, b); }
template <bool FLAT> DEV_INLINE uint32_t fe_wave_best(uint32_t v) { return FLAT ? wave_min_u32(v) : wave_max_u32(v); }
template <bool FLAT> DEV_INLINE uint32_t fe_row_best(uint32_t v) { return FLAT ? group_min_u32<16>(v) : group_max_u32<16>(v); }
#define FE_NMAX_ALL 0x7fffffff   // fe_pick_label's nmax: these kernels take the unlabelled (n_less_sharp + 1)-th pick as the reference does

// less_flat_scan of one picked sector, in position order (:279-285): the local indices [lsp, lep] of a ring whose flag bytes are sf and whose
// first staged point is rf, appended to st_lfs; all 64 lanes of a wavefront
DEV_INLINE void fe_less_flat_sector(const uint8_t* sf, int lsp, int lep, int rf, int* st_lfs, int& n_lfs) {
  const int lane = threadIdx.x & 63;
  for (int c0 = lsp; c0 <= lep; c0 += 64) {
    const int c = c0 + lane;
    const bool take = c <= lep && fe_less_flat_member(fe_flag_label(sf[c]));
    const unsigned long long m = __ballot(take);
    if (take) st_lfs[n_lfs + (int)__popcll(m & ((1ull << lane) - 1ull))] = c + rf;
    n_lfs += (int)__popcll(m);
  }
}

// one wavefront per (ring, slot).  Dynamic LDS: 3 bytes per ring point (column u16, the flag byte of fe_curv u8); the
// kernel's duration under load is set by how many rings fit a CU next to the other streams' workgroups.
// STDSORT (alego_params.sort_mode = 2): candidates with EQUAL curvature are taken in the order libstdc++'s std::sort leaves them in
// (laserOdometry.cpp:185 sorts with a comparator on the curvature alone) instead of by index.  The picks only ever ask for the
// best remaining candidate, so the sort itself is not needed — only, when several candidates tie for it, where std::sort's
// partition phase would have left each of them (stdsort_emu.h); that arrangement is computed once per sector, on the first tie.
template <int FE_T, bool STDSORT>
__global__ void __launch_bounds__(64) fe_pick(DevCtx d) {
  const int slot = blockIdx.y + d.slot0, ring = blockIdx.x, lane = threadIdx.x;
  __shared__ typename std::conditional<STDSORT, SortEmu<64 * FE_T>, char>::type s_emu;
  const size_t base = (size_t)slot * d.N;
  const alego_params& P = d.P;
  const int S = *ring_start_of(d, slot, ring), E = *ring_end_of(d, slot, ring);
  const int rf = S - 5, rl = E + 5;  // first / last point of this ring in the segmented cloud
  const int cnt = rl - rf + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char fe_smem[];
  uint16_t* s_col = reinterpret_cast<uint16_t*>(fe_smem);
  uint8_t* s_flag = fe_smem + 2 * (size_t)d.H;
  const float* cdv = d.cd + base + rf;  // fe_curv_key of it = the sort key
#pragma unroll 4
  for (int k = lane; k < cnt; k += 64) {   // the flag byte as fe_curv stored it (its jump bit is not looked at here: the columns are)
    s_col[k] = (uint16_t)d.seg_col[base + rf + k];
    s_flag[k] = d.fe_flag[base + rf + k];
  }
  __syncthreads();
  int* st = st_idx_of(d, slot, ring);
  int* st_sharp = st, *st_lsharp = st_idx_of(d, slot, ring, F_LSHARP), *st_flat = st_idx_of(d, slot, ring, F_FLAT), *st_lfs = st_idx_of(d, slot, ring, F_LFLAT);
  int n_sharp = 0, n_ls = 0, n_flat = 0, n_lfs = 0;
  const int NSEC = P.n_sectors, SR = P.suppress_radius;
  for (int j = 0; j < NSEC; ++j) {
    int sp, ep;
    fe_sector(P, S, E, j, sp, ep);
    if (fe_sector_skipped(sp, ep)) continue;
    const int lsp = sp - rf, lep = ep - rf;
    // Lane l owns the sector elements lsp + l + 64 t; their keys and candidate bits live in registers for the
    // whole sector, so an iteration of the greedy pick touches LDS only for the +-SR column test.
    uint32_t key[FE_T];
    uint32_t sharp_m = 0, flat_m = 0;
#pragma unroll
    for (int t = 0; t < FE_T; ++t) {
      const int c = lsp + lane + 64 * t;
      const bool ok = c <= lep;   // unconditional loads (clamped address): all of them in flight together
      const uint8_t f = s_flag[ok ? c : lsp];
      const uint32_t kv = fe_curv_key(cdv[ok ? c : lsp]);  // straight from HBM/L2: the LDS footprint decides how many rings fit a CU
      key[t] = ok ? kv : 0u;
      if (ok && fe_sharp_candidate(f)) sharp_m |= 1u << t;
      if (ok && fe_flat_candidate(f)) flat_m |= 1u << t;
    }
    // marks local index c and its fe_reach neighbours picked, in LDS for the later sectors and in the owners' candidate masks for this one
    auto mark = [&](int c, bool spread) {
      int nf = 0, nbk = 0;
      if (spread) {   // lanes 0 .. SR - 1 look forward, 32 .. 32 + SR - 1 backward
        bool bad = false;
        if (lane < SR) bad = fe_col_jump(s_col[c + lane + 1], s_col[c + lane], P.suppress_col_diff);
        else if (lane >= 32 && lane < 32 + SR) { const int l = lane - 32; bad = fe_col_jump(s_col[c - l - 1], s_col[c - l], P.suppress_col_diff); }
        const unsigned long long mb = __ballot(bad);
        const FeReach reach = fe_reach((unsigned)(mb & 0xffffffffull), (unsigned)(mb >> 32), SR);
        nf = reach.fwd; nbk = reach.bwd;
      }
      const int first = c - nbk, last = c + nf;
      if (lane <= last - first) s_flag[first + lane] |= FE_FLAG_PICKED;
      // the (single) owned element inside [first, last]
      const int off = (lane - (first - lsp)) & 63;
      const int ct = first + off;
      if (ct <= last && ct >= lsp && ct <= lep) { const uint32_t bit = 1u << ((ct - lsp - lane) / 64); sharp_m &= ~bit; flat_m &= ~bit; }
    };
    bool have_arr = false;
    auto sector_arrangement = [&]() {
      if constexpr (STDSORT) {
        const int n = lep - lsp + 1;
        __syncthreads();
        for (int i = lane; i < n; i += 64) s_emu.ak[i] = fe_curv_key(cdv[lsp + i]);   // |cd| bits order like the f64 curvature, equal iff it is
        __syncthreads();
        stdsort_arrangement(s_emu, n);
      }
    };
    // FLAT = false: sharp / less-sharp, descending curvature (:189-236); FLAT = true: flat, ascending, ground only (:238-277)
    auto pick = [&](auto flat_tag) {
      constexpr bool FLAT = decltype(flat_tag)::value;
      constexpr uint32_t NONE = fe_key_none<FLAT>();
      int picked_num = 0;
      while (true) {
        const uint32_t cand_m = FLAT ? flat_m : sharp_m;
        uint32_t bk = NONE;
        int bt = 0;
#pragma unroll
        for (int t = 0; t < FE_T; ++t) if (((cand_m >> t) & 1) && fe_scan_takes<FLAT>(key[t], bk)) { bk = key[t]; bt = t; }
        const uint32_t kbest = fe_wave_best<FLAT>(bk);
        if (kbest == NONE) break;
        // almost always exactly one lane holds the best key: its index comes through v_readlane; equal keys in several
        // lanes (fe_tie_takes) take the second reduction
        const unsigned long long tie = __ballot(cand_m && bk == kbest);
        int c = 0;
        bool by_arrangement = false;
        if constexpr (STDSORT) {
          int cnt = 0;
#pragma unroll
          for (int t = 0; t < FE_T; ++t) cnt += (((cand_m >> t) & 1) && key[t] == kbest) ? 1 : 0;
          const unsigned long long a1 = __ballot(cnt > 0), a2 = __ballot(cnt > 1);
          by_arrangement = a2 != 0 || (a1 & (a1 - 1)) != 0;
          if (by_arrangement) {   // fe_tie_takes_arranged, on fe_arranged_code
            if (!have_arr) { sector_arrangement(); have_arr = true; }
            uint32_t best = NONE;
#pragma unroll
            for (int t = 0; t < FE_T; ++t)
              if (((cand_m >> t) & 1) && key[t] == kbest) best = fe_better<FLAT>(best, fe_arranged_code<FLAT>((uint32_t)s_emu.pos[lane + 64 * t], (uint32_t)(lane + 64 * t)));
            c = lsp + (int)(fe_wave_best<FLAT>(best) & 0xFFFFu);
          }
        }
        if (by_arrangement) {
        } else if ((tie & (tie - 1)) == 0) {
          const int wl = __ffsll((long long)tie) - 1;
          c = lsp + wl + 64 * __builtin_amdgcn_readlane(bt, wl);
        } else {
          const uint32_t cand = (cand_m && bk == kbest) ? (uint32_t)(lsp + lane + 64 * bt) : NONE;
          c = (int)fe_wave_best<FLAT>(cand);
        }
        ++picked_num;
        int lab;
        bool spread, more;
        fe_pick_label<FLAT>(P, picked_num, FE_NMAX_ALL, lab, spread, more);
        if (lane == 0) {
          if (FLAT || lab) s_flag[c] = fe_flag_with_label(s_flag[c], lab);
          if (FLAT) st_flat[n_flat] = c + rf;
          else { if (lab == 2) st_sharp[n_sharp] = c + rf; if (lab) st_lsharp[n_ls] = c + rf; }
        }
        if (FLAT) ++n_flat;
        else { if (lab == 2) ++n_sharp; if (lab) ++n_ls; }
        mark(c, spread);
        if (!more) break;
      }
    };
    pick(std::false_type{});
    pick(std::true_type{});
    __syncthreads();
    fe_less_flat_sector(s_flag, lsp, lep, rf, st_lfs, n_lfs);
  }
  __syncthreads();
  for (int k = lane; k < cnt; k += 64) d.plabel[base + rf + k] = fe_flag_label(s_flag[k]);
  if (lane == 0) {
    int* c = st_cnt_of(d, slot, ring);
    c[F_SHARP] = n_sharp; c[F_LSHARP] = n_ls; c[F_FLAT] = n_flat; c[F_LFLAT] = n_lfs;
  }
}

// fe_pick4<FE_T>: the same greedy pick with FOUR rings per wavefront, one DPP row (16 lanes) each.  The per-pick
// overhead of the one-ring kernel (wave-wide arg-max, ballot, suppression window, uniform control flow: ~70 of its
// ~100 instructions per pick) is issued once for four rings; the reductions stay inside a DPP row.  Lane gl of a row owns
// the sector elements lsp + gl + 16 t (sector length <= 16 * FE_T).  Needs suppress_radius <= 5, what alego_create accepts and fe_reach looks at: the forward checks sit in
// lanes 0-7 of the row, the backward checks in lanes 8-15, and the 2 * radius + 1 marked elements get one lane each.  Dynamic LDS: 1 B per ring point, 4 rings.
// STDSORT (sort_mode 2): as in fe_pick — when several candidates of a row tie for the best curvature, the whole wavefront computes
// where libstdc++'s std::sort would have left that ring's sector (stdsort_emu.h), once per ring and sector, and the row picks by it.
#define FP_G 4
template <int FE_T, bool STDSORT = false>
__global__ void __launch_bounds__(64) fe_pick4(DevCtx d) {
  using mask_t = typename std::conditional<(FE_T > 32), unsigned long long, uint32_t>::type;
  __shared__ typename std::conditional<STDSORT, SortEmu<16 * FE_T>, char>::type s_emu;
  __shared__ uint16_t s_pos[STDSORT ? FP_G : 1][STDSORT ? 16 * FE_T : 1];
  static_assert(FE_T <= 64, "one candidate bit per owned element");
  const int slot = blockIdx.y + d.slot0, lane = threadIdx.x, g = lane >> 4, gl = lane & 15;
  const int ring0 = blockIdx.x * FP_G, ring = ring0 + g;
  const bool rv = ring < d.NS;
  const size_t base = (size_t)slot * d.N;
  const alego_params& P = d.P;
  extern __shared__ __attribute__((aligned(16))) unsigned char fe_smem[];
  // 1 B per ring point: the kernel's LDS footprint (one wavefront, four rings) is what limits how many of these workgroups —
  // and how much of the other stream groups' work — fit a CU.  The suppression only ever asks for fe_col_jump between a point
  // and the next: FE_FLAG_JUMP of the point's flag byte.
  uint8_t* s_flag = fe_smem;                                  // [FP_G][H]
  for (int r = 0; r < FP_G && ring0 + r < d.NS; ++r) {       // whole wavefront stages one ring after the other
    const int Sr = ring_start_of(d, slot, ring0)[r], Er = ring_end_of(d, slot, ring0)[r];
    const int rfr = Sr - 5, cntr = Er - Sr + 11;
    uint8_t* sf = s_flag + (size_t)r * d.H;
    // the flag byte of every point comes ready from fe_curv_chunk (fe_flag_of); the jump bit of the ring's last point compares with
    // the point itself in the reference's suppression loop (clamped index): cleared here
    const uint8_t* ff = d.fe_flag + base + rfr;
#pragma unroll 8
    for (int k = lane; k < cntr; k += 64) sf[k] = k == cntr - 1 ? (uint8_t)(ff[k] & ~FE_FLAG_JUMP) : ff[k];
  }
  __syncthreads();
  const int S = rv ? *ring_start_of(d, slot, ring) : 0, E = rv ? *ring_end_of(d, slot, ring) : 0;
  const int rf = S - 5;
  uint8_t* sf = s_flag + (size_t)g * d.H;
  int* st = st_idx_of(d, slot, rv ? ring : 0);
  int* st_sharp = st, *st_lsharp = st_idx_of(d, slot, rv ? ring : 0, F_LSHARP), *st_flat = st_idx_of(d, slot, rv ? ring : 0, F_FLAT);
  int n_sharp = 0, n_ls = 0, n_flat = 0;
  const int NSEC = P.n_sectors, SR = P.suppress_radius;
  for (int j = 0; j < NSEC; ++j) {
    int sp, ep;
    fe_sector(P, S, E, j, sp, ep);
    const bool act0 = rv && !fe_sector_skipped(sp, ep);
    if (!__any(act0)) continue;
    const int lsp = sp - rf, lep = ep - rf;
    uint32_t key[FE_T];
    mask_t sharp_m = 0, flat_m = 0;
#pragma unroll
    for (int t = 0; t < FE_T; ++t) {
      // unconditional loads (clamped address): all FE_T of them in flight together.  Behind a branch the compiler waited
      // for each load before it issued the next one: 19 global round trips per sector.
      const int c = lsp + gl + 16 * t;
      const bool ok = act0 && c <= lep;
      const uint8_t f = sf[ok ? c : 0];
      const uint32_t kv = fe_curv_key(d.cd[base + (ok ? rf + c : 0)]);
      key[t] = ok ? kv : 0u;
      const bool cs = fe_sharp_candidate(f), cf = fe_flat_candidate(f);   // (evaluated outside the && : behind it the compiler kept 16 - 40 more registers)
      if (ok && cs) sharp_m |= (mask_t)1 << t;
      if (ok && cf) flat_m |= (mask_t)1 << t;
    }
    // One greedy pick is a few hundred DEPENDENT instructions of a single wavefront (126 of them per ring quad): the loop body
    // is written branch-free.  LDS flag bytes are changed with no-return 32-bit atomics on the containing word (no read /
    // wait / write round trip; an operand of 0 or a clamped address makes a lane's update a no-op), loads use clamped
    // addresses, and only the list stores sit behind a (single) branch.
    unsigned* fw = reinterpret_cast<unsigned*>(s_flag);
    const int fo = g * d.H;                               // this ring's first flag byte
    // marks c and its fe_reach neighbours picked for the rows where `on`; `spread` rows look for column jumps first
    auto mark = [&](int c, bool on, bool spread) {
      const int role = gl & 7, rr = max(min(role, SR - 1), 0);   // lanes 0-7 look forward, 8-15 backward
      const int a = spread ? (gl < 8 ? c + rr : c - rr - 1) : 0;
      const bool bad = spread && role < SR && (sf[a] & FE_FLAG_JUMP);
      const unsigned long long mb = __ballot(bad);
      const unsigned gb = (unsigned)(mb >> (16 * g)) & 0xffffu;
      const FeReach reach = fe_reach(gb & 0xffu, gb >> 8, SR);
      const int nf = spread ? reach.fwd : 0, nbk = spread ? reach.bwd : 0;
      const int first = c - nbk, last = c + nf;
      const bool w = on && gl <= last - first;
      const int bo = fo + (w ? first + gl : 0);
      atomicOr(&fw[bo >> 2], (w ? (unsigned)FE_FLAG_PICKED : 0u) << ((bo & 3) * 8));
      const int off = (gl - (first - lsp)) & 15;   // the (single) owned element inside [first, last]
      const int ct = first + off;
      const mask_t bit = (on && ct <= last && ct >= lsp && ct <= lep) ? (mask_t)1 << (((ct - lsp - gl) >> 4) & (8 * (int)sizeof(mask_t) - 1)) : (mask_t)0;
      sharp_m &= ~bit; flat_m &= ~bit;
    };
    // the label bits of an unlabelled element hold label 0: x = 0 + 1 xor the new label + 1 turns them into it, 0 leaves them;
    // an element is labelled at most once (it is marked picked with it)
    auto relabel = [&](int c, unsigned x) {
      const int bo = fo + (x ? c : 0);
      atomicXor(&fw[bo >> 2], (x << FE_FLAG_LABEL_SHIFT) << ((bo & 3) * 8));
    };
    int* st_dummy = st_cnt_of(d, slot, rv ? ring : 0) + ST_DUMMY;   // unused field
    // (STDSORT) the sector arrangement of every ring whose row reports a tie and has none yet, ring by ring with all 64 lanes
    unsigned have_arr = 0;   // wavefront-uniform: bit r = ring r's arrangement of this sector is in s_pos[r]
    auto ring_arrangements = [&](bool tied) {
      if constexpr (STDSORT) {
        for (int r = 0; r < FP_G; ++r) {
          const bool want = __shfl((int)tied, 16 * r, 64) != 0;
          if (!want || ((have_arr >> r) & 1u)) continue;
          const int lsp_r = __shfl(lsp, 16 * r, 64), lep_r = __shfl(lep, 16 * r, 64), rf_r = __shfl(rf, 16 * r, 64);
          const int n = lep_r - lsp_r + 1;
          __syncthreads();
          for (int i = lane; i < n; i += 64) s_emu.ak[i] = fe_curv_key(d.cd[base + rf_r + lsp_r + i]);
          __syncthreads();
          stdsort_arrangement(s_emu, n);
          for (int i = lane; i < n; i += 64) s_pos[r][i] = s_emu.pos[i];
          __syncthreads();
          have_arr |= 1u << r;
        }
      }
    };
    // FLAT = false: sharp / less-sharp, descending curvature (:189-236); FLAT = true: flat, ascending, ground only (:238-277)
    // (what the loop only reads is captured by value: through references the sort_mode 2 instances kept 20 - 24 more registers and lost a wavefront per SIMD.
    //  CAREFUL: key, P and the helper lambdas are COPIES here — the helpers still reach sharp_m / flat_m / have_arr through their own references — so a
    //  local of the sector that the loop is to change has to be named in the capture list by reference, or the loop changes a copy.)
    auto pick = [=, &sharp_m, &flat_m, &n_sharp, &n_ls, &n_flat](auto flat_tag) {
      constexpr bool FLAT = decltype(flat_tag)::value;
      constexpr uint32_t NONE = fe_key_none<FLAT>();
      int picked_num = 0;
      bool act = act0;
      while (true) {
        const mask_t cand_m = FLAT ? flat_m : sharp_m;
        uint32_t bk = NONE;
        int bt = 0;
#pragma unroll
        for (int t = 0; t < FE_T; ++t) if (((cand_m >> t) & 1) && fe_scan_takes<FLAT>(key[t], bk)) { bk = key[t]; bt = t; }
        if (!act) bk = NONE;
        const uint32_t kbest = fe_row_best<FLAT>(bk);
        act = act && kbest != NONE;
        if (!__any(act)) break;
        int c = (int)fe_row_best<FLAT>(bk == kbest ? (uint32_t)(lsp + gl + 16 * bt) : NONE);   // fe_tie_takes
        if constexpr (STDSORT) {
          int cnt = 0;
#pragma unroll
          for (int t = 0; t < FE_T; ++t) cnt += (((cand_m >> t) & 1) && key[t] == kbest) ? 1 : 0;
          if (!act) cnt = 0;
          const bool tied = group_max_u32<16>((uint32_t)cnt) > 1u || __popc((unsigned)(__ballot(cnt > 0) >> (16 * g)) & 0xffffu) > 1;
          if (__any(tied)) {
            ring_arrangements(tied);
            uint32_t best = NONE;   // fe_tie_takes_arranged, on fe_arranged_code
#pragma unroll
            for (int t = 0; t < FE_T; ++t)
              if (((cand_m >> t) & 1) && key[t] == kbest) best = fe_better<FLAT>(best, fe_arranged_code<FLAT>((uint32_t)s_pos[g][gl + 16 * t], (uint32_t)(gl + 16 * t)));
            const int ca = lsp + (int)(fe_row_best<FLAT>(tied ? best : NONE) & 0xFFFFu);
            c = tied ? ca : c;
          }
        }
        picked_num += act ? 1 : 0;
        int lab;
        bool spread, more;
        fe_pick_label<FLAT>(P, picked_num, FE_NMAX_ALL, lab, spread, more);
        const bool w1 = act && gl == 0 && lab != 0;
        relabel(c, w1 ? 1u ^ (unsigned)(lab + 1) : 0u);
        if (w1) {
          if (FLAT) st_flat[n_flat] = c + rf;
          else {
            int* ps = lab == 2 ? st_sharp + n_sharp : st_dummy;
            *ps = c + rf;
            st_lsharp[n_ls] = c + rf;
          }
        }
        if (FLAT) n_flat += act ? 1 : 0;
        else { n_sharp += (act && lab == 2) ? 1 : 0; n_ls += (act && lab) ? 1 : 0; }
        mark(c, act, act && spread);
        act = act && more;
      }
    };
    pick(std::false_type{});
    pick(std::true_type{});
  }
  __syncthreads();
  if (rv && gl == 0) {
    int* c = st_cnt_of(d, slot, ring);
    c[F_SHARP] = n_sharp; c[F_LSHARP] = n_ls; c[F_FLAT] = n_flat;
  }
  // ---- less_flat_scan and the labels, one ring after the other with all 64 lanes.
  // A sector's labels only change while that sector is picked, so reading them at the end is the same as reading them
  // after the sector.
  for (int r = 0; r < FP_G && ring0 + r < d.NS; ++r) {
    const int Sr = ring_start_of(d, slot, ring0)[r], Er = ring_end_of(d, slot, ring0)[r];
    const int rfr = Sr - 5, cntr = Er - Sr + 11;
    const uint8_t* sfr = s_flag + (size_t)r * d.H;
    int* st_lfs = st_idx_of(d, slot, (size_t)ring0 + r, F_LFLAT);
    int n_lfs = 0;
    for (int j = 0; j < NSEC; ++j) {
      int sp, ep;
      fe_sector(P, Sr, Er, j, sp, ep);
      if (fe_sector_skipped(sp, ep)) continue;
      fe_less_flat_sector(sfr, sp - rfr, ep - rfr, rfr, st_lfs, n_lfs);
    }
    for (int k = lane; k < cntr; k += 64) d.plabel[base + rfr + k] = fe_flag_label(sfr[k]);
    if (lane == 0) st_cnt_of(d, slot, (size_t)ring0 + r)[F_LFLAT] = n_lfs;
  }
}

// one block per (ring, slot): pcl::VoxelGrid on the ring's less_flat_scan.
// Consecutive points of a ring mostly fall into the same 0.4 m voxel, so the (voxel id, position) sort is done on
// RUNS of equal consecutive voxel ids (a few hundred per ring instead of ~1000 points): rank-by-counting of the
// runs in LDS, then the first run of every voxel accumulates all runs of that voxel in order — the same f32
// summation order as a stable sort of the points.  Dynamic LDS: 10 B per ring point (+ 4 KB of bucket counters): the
// number of these workgroups that fit a CU decides the kernel's duration.
#ifdef ALEGO_TIMING
__device__ long long fv_times[12];
extern "C" void alego_fv_times(long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(fv_times), sizeof(long long) * 12); }
#define FV_TICK(k) do { if (threadIdx.x == 0 && blockIdx.x == 8 && blockIdx.y == 0) fv_times[k] = wall_clock64(); } while (0)
#else
#define FV_TICK(k)
#endif
#ifndef FV_NB
#define FV_NB 256
#endif
#ifndef FV_BLOCK
#define FV_BLOCK 256   // threads per ring
#endif
#ifndef FV_STAGE
#define FV_STAGE 1     // 1: the ring's candidate points are gathered once into LDS (26 B per column); 0: every pass gathers them from HBM / L2 (10 B per column)
#endif
// (ranking the ~300 runs of a ring by counting — every run sweeps all runs in LDS — was measured: 346 k -> 317 k scans/s.  The
//  pipeline as a whole is VALU-issue bound; 90 k compares per ring cost more than the bucket tables' latency.)
#define FV_LDS_PER_COL (FV_STAGE ? 26 : 10)
// Points staged in LDS per ring: a ring of H columns holds ~0.6 H less_flat_scan points (the rest are empty, ground-only or picked cells); the
// staging area is sized for 0.72 H of them and a fuller ring reads its tail from the L2 on every pass.  10 H + 16 x 0.72 H + 2.2 KB = 40.9 KB at
// H = 1800: FOUR rings per CU instead of three (26 H + 4.2 KB = 51 KB).  Same run, scans/s: 512 buckets + everything staged 395 k; 512 buckets +
// 0.64 H staged 406 k; 256 buckets + 0.72 H staged 407 k; nothing staged (three gathers through the L2 per point) 402 k.
#ifndef FV_CAP_PCT
#define FV_CAP_PCT 72
#endif
// Wide images (H = 4000: the key arrays alone are 40 KB) stage less or nothing, so that the workgroup stays near 40 KB: a ring of 16 x 4000 with
// everything staged took 88 KB — one workgroup per CU, fe_voxel a quarter of that geometry's device time.
__host__ __device__ inline int fv_stage_cap(int H) {
  if (!FV_STAGE) return 0;
  const int by_pct = (H * FV_CAP_PCT / 100 + 15) & ~15, by_lds = (40960 - 2200 - 10 * H) / 16;
  return by_lds <= 0 ? 0 : (by_pct < by_lds ? by_pct : (by_lds & ~15));
}
static size_t fv_lds_bytes(int H) { return (size_t)10 * H + (size_t)16 * fv_stage_cap(H); }
#define FV_U 4    // gathers kept in flight per thread
__global__ void __launch_bounds__(FV_BLOCK) fe_voxel(DevCtx d) {
  const int slot = blockIdx.y + d.slot0, ring = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)slot * d.N;
  int* cnts = st_cnt_of(d, slot, ring);
  const int n = cnts[F_LFLAT];
  const int* lfs = st_idx_of(d, slot, ring, F_LFLAT);
  float4* out = st_lfds_of(d, slot, ring);
  const float4* seg = d.seg_lo + base;
  extern __shared__ __attribute__((aligned(16))) unsigned char fv_smem[];
  float4* s_pt = reinterpret_cast<float4*>(fv_smem);                            // the ring's less_flat_scan points, gathered ONCE [cap] (FV_STAGE)
  const int cap = fv_stage_cap(d.H);
  unsigned char* fv2 = fv_smem + (size_t)16 * cap;
  auto point = [&](int i) -> float4 { if (i < cap) return s_pt[i]; return seg[lfs[i]]; };
  uint32_t* s_key = reinterpret_cast<uint32_t*>(fv2);                           // voxel id per point      [H]
  uint32_t* s_rvid = s_key;                                                     // voxel id per run, compacted in place (run r <= its first point)
  uint16_t* s_rstart = reinterpret_cast<uint16_t*>(fv2 + 4 * (size_t)d.H);      // first point of the run  [H]
  uint16_t* s_order = reinterpret_cast<uint16_t*>(fv2 + 6 * (size_t)d.H);       // runs sorted by (voxel id, run) [H]
  uint16_t* s_tmp = reinterpret_cast<uint16_t*>(fv2 + 8 * (size_t)d.H);         // runs dealt into buckets [H]
  __shared__ float s_red[6][FV_BLOCK / 64];
  __shared__ int s_scan[FV_BLOCK / 64];
  __shared__ int s_boff[FV_NB + 1], s_bcur[FV_NB + 1];
  if (n == 0) { if (tid == 0) cnts[ST_LFDS] = 0; return; }
  const float inv = 1.0f / d.P.less_flat_leaf;
  FV_TICK(0);
  // getMinMax3D
  float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  // gathers through the index list: FV_U index loads, then FV_U point loads in flight together
  for (int i0 = tid; i0 < n; i0 += FV_BLOCK * FV_U) {
    int ix[FV_U];
    float4 pt[FV_U];
#pragma unroll
    for (int u = 0; u < FV_U; ++u) ix[u] = lfs[min(i0 + u * FV_BLOCK, n - 1)];
#pragma unroll
    for (int u = 0; u < FV_U; ++u) pt[u] = seg[ix[u]];
#pragma unroll
    for (int u = 0; u < FV_U; ++u) {   // (a clamped duplicate of the last point does not change min / max)
      if (i0 + u * FV_BLOCK < min(n, cap)) s_pt[i0 + u * FV_BLOCK] = pt[u];   // every later pass reads the point from LDS: one global round trip instead of three
      vgr_box_add(mn, mx, pt[u]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bfly_minmax_f32(mn[a], mx[a]);
    if ((tid & 63) == 0) { s_red[a][tid >> 6] = mn[a]; s_red[3 + a][tid >> 6] = mx[a]; }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = s_red[a][0]; mx[a] = s_red[3 + a][0];
#pragma unroll
    for (int w = 1; w < FV_BLOCK / 64; ++w) { mn[a] = fminf(mn[a], s_red[a][w]); mx[a] = fmaxf(mx[a], s_red[3 + a][w]); }
  }
  if (vgr_leaf_too_small(mn, mx, inv)) {  // "leaf size too small": the input is returned unchanged
    for (int i = tid; i < n; i += FV_BLOCK) out[i] = point(i);
    if (tid == 0) cnts[ST_LFDS] = n;
    return;
  }
  FV_TICK(1);
  const VgrGeom g = vgr_geom(mn, mx, inv);
#pragma unroll 4
  for (int i = tid; i < n; i += FV_BLOCK) s_key[i] = vgr_id(g, point(i), inv);
  __syncthreads();
  FV_TICK(2);
  // the heads of a chunk of FV_BLOCK positions numbered in position order: -> heads before this thread's, *tot = heads of the chunk (ballots: a
  // head is a bit, and wave.h's block_excl_scan would pay six shuffle steps for it); one barrier inside, the caller's barrier ends the chunk
  auto heads_before = [&](bool head, int* tot) -> int {
    const unsigned long long m = __ballot(head);
    if ((tid & 63) == 0) s_scan[tid >> 6] = (int)__popcll(m);
    __syncthreads();
    int woff = 0, t = 0;
#pragma unroll
    for (int w = 0; w < FV_BLOCK / 64; ++w) { if (w < (tid >> 6)) woff += s_scan[w]; t += s_scan[w]; }
    *tot = t;
    return woff + (int)__popcll(m & ((1ull << (tid & 63)) - 1ull));
  };
  // runs of consecutive equal voxel ids
  int nruns = 0;
  for (int c0 = 0; c0 < n; c0 += FV_BLOCK) {
    const int i = c0 + tid;
    const uint32_t mykey = i < n ? s_key[i] : 0u;   // read before the barrier: the run ids are compacted into the same array
    const bool head = i < n && (i == 0 || mykey != s_key[i - 1]);
    int tot;
    const int before = heads_before(head, &tot);
    if (head) {
      const int r = nruns + before;
      s_rvid[r] = mykey;
      s_rstart[r] = (uint16_t)i;
    }
    nruns += tot;
    __syncthreads();
  }
  FV_TICK(3);
  // Order the runs by (voxel id, run index).  Voxel ids are bounded by the grid size T, so the runs are first dealt
  // into <= FV_NB buckets that are monotone in the voxel id (LDS atomics; arbitrary order inside a bucket), then
  // every run ranks itself among the one or two runs of its bucket — instead of against all runs of the ring.
  {
    const FeBuckets bk = fe_buckets(g.T, FV_NB);
    fe_buckets_clear<FV_BLOCK>(bk.nb, s_boff);
    __syncthreads();
    for (int r = tid; r < nruns; r += FV_BLOCK) atomicAdd(&s_boff[fe_bucket_of(bk, s_rvid[r]) + 1], 1);
    __syncthreads();
    fe_buckets_scan<FV_BLOCK, FV_NB>(bk.nb, s_boff, s_bcur, s_scan);
    __syncthreads();
    for (int r = tid; r < nruns; r += FV_BLOCK) s_tmp[atomicAdd(&s_bcur[fe_bucket_of(bk, s_rvid[r])], 1)] = (uint16_t)r;
    __syncthreads();
    for (int t = tid; t < nruns; t += FV_BLOCK) {
      const int r = s_tmp[t];
      const uint32_t v = s_rvid[r];
      const int b = fe_bucket_of(bk, v);
      const int bs = s_boff[b], be = s_boff[b + 1];
      int rank = bs;
      for (int q = bs; q < be; ++q) { const int o = s_tmp[q]; const uint32_t u = s_rvid[o]; rank += (u < v) || (u == v && o < r); }
      s_order[rank] = (uint16_t)r;
    }
  }
  __syncthreads();
  FV_TICK(4);
  // first run of every voxel -> output rank; it accumulates all runs of the voxel in order
  int nvox = 0;
  for (int c0 = 0; c0 < nruns; c0 += FV_BLOCK) {
    const int j = c0 + tid;
    const bool head = j < nruns && (j == 0 || s_rvid[s_order[j]] != s_rvid[s_order[j - 1]]);
    int tot;
    const int before = heads_before(head, &tot);
    if (head) {
      const int rank = nvox + before;
      const uint32_t vid = s_rvid[s_order[j]];
      float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
      int c = 0;
      for (int jj = j; jj < nruns && s_rvid[s_order[jj]] == vid; ++jj) {
        const int r = s_order[jj], i0 = s_rstart[r], len = (r + 1 < nruns ? (int)s_rstart[r + 1] : n) - i0;
        for (int i = i0; i < i0 + len; ++i) { const float4 q = point(i); sx += q.x; sy += q.y; sz += q.z; si += q.w; ++c; }   // strictly in order
      }
      const float fn = (float)c;
      out[rank] = make_float4(sx / fn, sy / fn, sz / fn, si / fn);
    }
    nvox += tot;
    __syncthreads();
  }
  if (tid == 0) cnts[ST_LFDS] = nvox;
  FV_TICK(5);
}

// fe_collect = ring-ascending concatenation of the four feature clouds (:199-205,:245,:293) + the bounding boxes of every LO_CH
// consecutive less_flat / less_sharp points for the next scan's LaserOdometry (kernels_lo.hip), one workgroup per stream (was
// fe_gather + fe_boxes: 16 + 48 workgroups per stream in two launches, the second one re-reading what the first had written).
// Output point i of a cloud belongs to the ring r with off[r] <= i < off[r + 1] (binary search in the per-ring prefix, LDS);
// 32 consecutive threads hold the 32 points of a box.
#define FC_T 512
__global__ void __launch_bounds__(FC_T) fe_collect(DevCtx d) {
  const int slot = blockIdx.x + d.slot0, tid = threadIdx.x;
  const size_t fb = fbuf(slot, cur_in_flight(d, slot));
  const int NS = d.NS;
  __shared__ int s_off[4][65], s_lf[2][65];   // fe_concat_picks' offsets; less_flat: first point, first box of every ring
  if (tid < 64) {
    const int c = tid < NS ? st_cnt_of(d, slot, 0)[tid * ST_W + ST_LFDS] : 0;
    fe_ring_offsets(c, s_lf[0]);
    fe_ring_offsets((c + LO_CH - 1) / LO_CH, s_lf[1]);
  }
  fe_concat_picks<FC_T>(d, slot, fb, s_off, false);   // (its barrier stands behind s_lf too; fe_pick / fe_pick4 wrote cloud_label_)
  // this kernel's own: the less_flat cloud (the per-ring VoxelGrid outputs of fe_voxel) and its boxes
  if (tid <= NS) {
    ring_off_of(d, fb, RO_LFLAT)[tid] = s_lf[0][tid < NS ? tid : 64];
    ring_boff_of(d, fb, RO_LFLAT)[tid] = s_lf[1][tid < NS ? tid : 64];
  }
  if (tid == 0) feat_cnt_of(d, fb)[F_LFLAT] = s_lf[0][64];
  fe_concat_cloud<FC_T>(NS, s_lf[0], s_lf[1], feat_of(d, F_LFLAT, fb), lo_box_of(d, lo_row(fb, box_set_of(F_LFLAT))),
                        [&](int r, int j, int) -> float4 { return st_lfds_of(d, slot, r)[j]; });
}

// alego_debug_std_sort: the emulation on its own (one wavefront, up to 4096 keys)
#define STDSORT_PROBE_MAX 4096
__global__ void __launch_bounds__(64) stdsort_probe(const uint32_t* keys, int n, int depth_limit, int* pos_out) {
  __shared__ SortEmu<STDSORT_PROBE_MAX> E;
  for (int i = threadIdx.x; i < n; i += 64) E.ak[i] = keys[i];
  __syncthreads();
  stdsort_arrangement(E, n, depth_limit);
  for (int i = threadIdx.x; i < n; i += 64) pos_out[i] = E.pos[i];
}
int launch_stdsort_probe(const uint32_t* keys, int n, int depth_limit, int* pos_out, hipStream_t st) {
  if (n > STDSORT_PROBE_MAX) return -1;
  hipLaunchKernelGGL(stdsort_probe, dim3(1), dim3(64), 0, st, keys, n, depth_limit, pos_out);
  return 0;
}

void launch_fe_curv_debug(const DevCtx& d, hipStream_t st) { ALEGO_LAUNCH(fe_curv, dim3((d.N + FE_CW - 1) / FE_CW, d.n_launch), dim3(FE_BLOCK), 0, st, d); }

void launch_fe(const DevCtx& d, hipStream_t st) {
  if (fe_fused_eligible(d)) { launch_fe_fused(d, st); launch_lo_grid(d, st); return; }   // fe_cand + fe_pickc + fe_ring_out; below: the four-kernel path (ALEGO_FE_FUSED=0, sort_mode 2)
  // dynamic LDS above 64 KB has to be requested explicitly (fe_voxel: 26 B per column, horizon_scan <= 4096)
  static const bool cfg = hipFuncSetAttribute(reinterpret_cast<const void*>(fe_voxel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fv_lds_bytes(FE_MAXH)) == hipSuccess;
  (void)cfg;
  ALEGO_LAUNCH(fe_curv, dim3((d.N + FE_CW - 1) / FE_CW, d.n_launch), dim3(FE_BLOCK), 0, st, d);
  // the longest sector holds at most ceil(H / n_sectors) + 1 points
  const int sector_max = (d.H + d.P.n_sectors - 1) / (d.P.n_sectors > 0 ? d.P.n_sectors : 1) + 2;
  // (padding this allocation by 16 KB cost 7 % of the whole pipeline: the LDS footprint decides how many rings share a CU)
  const int extra = 0;
  const bool one_ring = d.opt_fe_pick1 || d.P.suppress_radius > 7 || sector_max > 16 * 43;   // (2 * radius + 1 marked elements <= 16 lanes)
  const dim3 g4((d.NS + FP_G - 1) / FP_G, d.n_launch);
  const size_t lds4 = (size_t)FP_G * d.H;
  const bool ss = d.P.sort_mode == 2;
  if (!one_ring && ss && sector_max <= 16 * 19) { ALEGO_LAUNCH((fe_pick4<19, true>), g4, dim3(64), lds4, st, d); }
  else if (!one_ring && ss && sector_max <= 16 * 24) { ALEGO_LAUNCH((fe_pick4<24, true>), g4, dim3(64), lds4, st, d); }
  else if (!one_ring && ss) { ALEGO_LAUNCH((fe_pick4<43, true>), g4, dim3(64), lds4, st, d); }
  else if (!one_ring && sector_max <= 16 * 19) { ALEGO_LAUNCH(fe_pick4<19>, g4, dim3(64), lds4, st, d); }
  else if (!one_ring && sector_max <= 16 * 24) { ALEGO_LAUNCH(fe_pick4<24>, g4, dim3(64), lds4, st, d); }
  else if (!one_ring) { ALEGO_LAUNCH(fe_pick4<43>, g4, dim3(64), lds4, st, d); }
  else if (d.P.sort_mode == 2 && sector_max <= 64 * 6) { ALEGO_LAUNCH((fe_pick<6, true>), dim3(d.NS, d.n_launch), dim3(64), (size_t)3 * d.H, st, d); }
  else if (d.P.sort_mode == 2) { ALEGO_LAUNCH((fe_pick<12, true>), dim3(d.NS, d.n_launch), dim3(64), (size_t)3 * d.H, st, d); }
  else if (sector_max <= 64 * 6) { ALEGO_LAUNCH((fe_pick<6, false>), dim3(d.NS, d.n_launch), dim3(64), (size_t)3 * d.H + extra, st, d); }
  else { ALEGO_LAUNCH((fe_pick<12, false>), dim3(d.NS, d.n_launch), dim3(64), (size_t)3 * d.H, st, d); }
  ALEGO_LAUNCH(fe_voxel, dim3(d.NS, d.n_launch), dim3(FV_BLOCK), fv_lds_bytes(d.H), st, d);
  ALEGO_LAUNCH(fe_collect, dim3(d.n_launch), dim3(FC_T), 0, st, d);
  launch_lo_grid(d, st);
}
