// fe_rules_check — csrc/fe_rules.h on the host: every rule of the feature pick against the reference's loops (laserOdometry.cpp:122-285) written out
// plainly here, the mask forms against the per-point forms, and a greedy best-remaining pick built from the header's rules alone against the reference's
// sort-then-scan on random rings with many tied curvatures.  Built with -ffp-contract=off, ASan and UBSan: no shift or index of the header leaves its type.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "fe_rules.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static int rnd(int n) { return (int)(rnd64() % (uint64_t)n); }

// ---- sectors (:177-178, LO.cpp:245-249) ----
static long long sectors() {
  long long n = 0;
  const int kNsec[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 24};
  const int kS[] = {4, 5, 17, 1000, 28000};
  for (int formula = 0; formula < 2; ++formula)
    for (int nsec : kNsec)
      for (int S : kS)
        for (int E = S - 10; E <= S + 80; ++E) {   // E = S - 10: what ImageProjection leaves for a ring without a point
          volatile int nv = nsec;                     // (a divisor the compiler cannot see: the general form even where nsec is 6)
          int prev_ep = S - 1;
          for (int j = 0; j < nsec; ++j, ++n) {
            int want_sp, want_ep;
            if (formula == 0) { want_sp = (S * (nv - j) + E * j) / nv; want_ep = (S * (nv - 1 - j) + E * (j + 1)) / nv - 1; }
            else { const int diff = E - S; want_sp = S + j * diff / nv; want_ep = S + (j + 1) * diff / nv - 1; }
            int sp, ep;
            fe_sector(formula, nsec, S, E, j, sp, ep);
            CHECK(sp == want_sp && ep == want_ep, "sector: formula %d nsec %d S %d E %d j %d: [%d, %d] want [%d, %d]", formula, nsec, S, E, j, sp, ep, want_sp, want_ep);
            CHECK(sp == fe_sector_start(formula, nsec, S, E, j), "fe_sector's sp is fe_sector_start");
            CHECK(sp == prev_ep + 1, "sectors contiguous: formula %d nsec %d S %d E %d j %d: sp %d after ep %d", formula, nsec, S, E, j, sp, prev_ep);
            if (E >= S) CHECK(ep >= sp - 1, "a sector of a ring with points is never shorter than empty");
            CHECK(fe_sector_skipped(sp, ep) == (ep - sp + 1 < 2), "a sector of fewer than two points is skipped");
            prev_ep = ep;
          }
          CHECK(prev_ep == E - 1, "sectors tile [S, E - 1]: formula %d nsec %d S %d E %d: last ep %d", formula, nsec, S, E, prev_ep);
          CHECK(fe_sector_start(formula, nsec, S, E, nsec) == E, "sector n_sectors starts at E");
        }
  return n;
}

// ---- curvature (:122-129) and markOccludedPoints (:131-159) ----
static unsigned occl_written_out(int f32, double depth, int cold, double ratio, float rm, float r0, float r1, int c0, int c1) {
  unsigned m = 0;
  const int col_diff = abs(c0 - c1);
  bool first = false;
  if (f32) {   // LO.cpp:203-204: float depth1 / depth2
    const float depth1 = r0, depth2 = r1;
    if (col_diff < cold) {
      if (depth1 - depth2 > depth) { m |= 1; first = true; }
      else if (depth2 - depth1 > depth) m |= 2;
    }
    if (!first) {
      const double diff1 = fabsf(rm - depth1), diff2 = fabsf(depth2 - depth1);
      if (diff1 > ratio * r0 && diff2 > ratio * r0) m |= 4;
    }
  } else {
    const double depth1 = r0, depth2 = r1;
    if (col_diff < cold) {
      if (depth1 - depth2 > depth) { m |= 1; first = true; }
      else if (depth2 - depth1 > depth) m |= 2;
    }
    if (!first) {
      const double diff1 = fabs(rm - depth1), diff2 = fabs(depth2 - depth1);
      if (diff1 > ratio * r0 && diff2 > ratio * r0) m |= 4;
    }
  }
  return m;
}
static long long curvature_and_marks() {
  long long n = 0;
  for (int it = 0; it < 20000; ++it, ++n) {
    float r[11];
    for (float& v : r) v = 1.0f + (float)rnd(1 << 20) / 8192.0f + (rnd(4) ? 0.f : 1e-3f * (float)rnd(1000));
    volatile float acc = r[0];   // strictly left to right, every partial sum rounded to f32
    acc = acc + r[1]; acc = acc + r[2]; acc = acc + r[3]; acc = acc + r[4];
    { volatile float t = r[5] * 10; acc = acc - t; }
    acc = acc + r[6]; acc = acc + r[7]; acc = acc + r[8]; acc = acc + r[9]; acc = acc + r[10];
    const float cd = fe_curv_sum(r + 5);
    CHECK(fe_f32_bits(cd) == fe_f32_bits(acc), "11-tap sum: %a want %a", cd, (float)acc);
    CHECK(fe_curvature(cd) == (double)cd * (double)cd, "curvature is the f64 square of the f32 sum");
    const float cd2 = rnd(3) ? -cd : cd * (1.0f + (float)rnd(3) * 1e-6f);
    CHECK((fe_curv_key(cd) < fe_curv_key(cd2)) == (fe_curvature(cd) < fe_curvature(cd2)) && (fe_curv_key(cd) == fe_curv_key(cd2)) == (fe_curvature(cd) == fe_curvature(cd2)),
          "the key orders like the curvature: %a %a", cd, cd2);
    CHECK(fe_curv_edge(fe_curvature(cd), 0.1) == ((double)cd * cd > 0.1) && fe_curv_surf(fe_curvature(cd), 0.1) == ((double)cd * cd < 0.1), "thresholds");
    // marks: ranges a few centimetres to metres apart, columns either side of the limit
    const float r0 = 2.0f + (float)rnd(4000) / 100.0f;
    const float step[] = {0.f, 0.01f, 0.3f, 0.49999f, 0.5f, 0.50001f, 0.7f, 3.0f};
    const float rm = r0 + (rnd(2) ? 1.f : -1.f) * step[rnd(8)] * (rnd(2) ? 1.f : 0.04f * r0), r1 = r0 + (rnd(2) ? 1.f : -1.f) * step[rnd(8)] * (rnd(2) ? 1.f : 0.04f * r0);
    const int c0 = rnd(1800), c1 = c0 + rnd(25) - 12;
    for (int f32 = 0; f32 < 2; ++f32) {
      const unsigned got = fe_occl_marks(f32, 0.5, 10, 0.02, rm, r0, r1, c0, c1), want = occl_written_out(f32, 0.5, 10, 0.02, rm, r0, r1, c0, c1);
      CHECK(got == want, "occlusion marks (occl_f32 %d): r %a %a %a cols %d %d: %u want %u", f32, rm, r0, r1, c0, c1, got, want);
    }
    CHECK(fe_col_jump(c0, c1, 10) == (abs(c1 - c0) > 10), "column jump");
  }
  CHECK(fe_has_taps(5, 100) && !fe_has_taps(4, 100) && fe_has_taps(94, 100) && !fe_has_taps(95, 100) && !fe_has_taps(5, 10), "points 5 .. M - 6 have the taps");
  return n;
}

// ---- a point is picked: the lane-mask form against the per-point form, across chunk boundaries ----
static long long picked_masks() {
  long long n = 0;
  const int NCH = 5, N = 64 * NCH;
  for (int it = 0; it < 400; ++it) {
    std::vector<uint8_t> m(N + 10, 0);   // 5 entries of margin either side
    const int dens = 1 + rnd(12);
    for (int i = 0; i < N; ++i) m[5 + i] = (uint8_t)((rnd(dens) ? 0 : 1) | (rnd(dens) ? 0 : 2) | (rnd(dens + 3) ? 0 : 4));
    uint64_t a[NCH + 2] = {0}, b[NCH + 2] = {0}, c[NCH + 2] = {0};   // chunk k at [k + 1]
    for (int i = 0; i < N; ++i) {
      if (m[5 + i] & FE_OCCL_A) a[i / 64 + 1] |= 1ull << (i % 64);
      if (m[5 + i] & FE_OCCL_B) b[i / 64 + 1] |= 1ull << (i % 64);
      if (m[5 + i] & FE_OCCL_C) c[i / 64 + 1] |= 1ull << (i % 64);
    }
    for (int i = 0; i < N; ++i, ++n) {
      const int k = i / 64 + 1;
      bool want = (m[5 + i] & 4) != 0;   // written out: A over [i, i + 5], B over [i - 5, i - 1], C at i
      for (int l = 0; l <= 5; ++l) want = want || (m[5 + i + l] & 1);
      for (int l = 1; l <= 5; ++l) want = want || (m[5 + i - l] & 2);
      const bool per_point = fe_point_picked(m.data() + 5 + i), on_masks = fe_point_picked(a[k], a[k + 1], b[k - 1], b[k], c[k], i % 64);
      CHECK(per_point == want && on_masks == want, "picked at %d: per point %d, on masks %d, want %d", i, per_point, on_masks, want);
    }
  }
  return n;
}

// ---- the flag byte ----
static long long flags() {
  long long n = 0;
  for (unsigned f = 0; f < 256; ++f, ++n) {
    const bool picked = f & 1, ground = f & 2, edge = f & 4, surf = f & 8, jump = f & 64;
    const int label = (int)((f >> 4) & 3) - 1;
    CHECK(fe_sharp_candidate(f) == (!picked && !ground && edge) && fe_sharp_candidate(f) == fe_sharp_candidate(picked, ground, edge), "sharp candidate, flag %u", f);
    CHECK(fe_flat_candidate(f) == (!picked && ground && surf) && fe_flat_candidate(f) == fe_flat_candidate(picked, ground, surf), "flat candidate, flag %u", f);
    CHECK(fe_flag_label(f) == label, "label of flag %u", f);
    if (!(f & 128)) CHECK(fe_flag_of(picked, ground, edge, surf, label, jump) == f, "fe_flag_of rebuilds flag %u", f);
    for (int lab = -1; lab <= 2; ++lab) {
      const unsigned g = fe_flag_with_label(f, lab);
      CHECK(fe_flag_label(g) == lab && (g & 0xCF) == (f & 0xCF), "fe_flag_with_label(%u, %d) = %u", f, lab, g);
    }
  }
  CHECK(FE_FLAG_PICKED == 1 && FE_FLAG_GROUND == 2 && FE_FLAG_EDGE == 4 && FE_FLAG_SURF == 8 && FE_FLAG_LABEL == 0x30 && FE_FLAG_JUMP == 64, "the bits of the flag byte");
  CHECK(fe_less_flat_member(-1) && fe_less_flat_member(0) && !fe_less_flat_member(1) && !fe_less_flat_member(2), "less_flat_scan: label <= 0");
  return n;
}

// ---- suppression reach (:211-234) against the reference's two loops ----
static long long reach() {
  long long n = 0;
  for (unsigned jf = 0; jf < 32; ++jf)
    for (unsigned jb = 0; jb < 32; ++jb)
      for (int R = 0; R <= 5; ++R, ++n) {
        // columns around a pick at index 8: a jump of 11 where the pattern has a bit, a step of 1 elsewhere
        int col[17];
        col[0] = 0;
        for (int i = 1; i < 17; ++i) {
          bool jump = false;                                    // between i - 1 and i
          if (i - 1 >= 8 && i - 1 - 8 < 5) jump = (jf >> (i - 1 - 8)) & 1;   // between c + l and c + l + 1: bit l
          if (i <= 8 && 8 - i < 5) jump = (jb >> (8 - i)) & 1;               // between c - l - 1 and c - l: bit l
          col[i] = col[i - 1] + (jump ? 11 : 1);
        }
        int fwd = 0, bwd = 0;
        for (int l = 1; l <= R; ++l) { if (abs(col[8 + l] - col[8 + l - 1]) > 10) break; fwd = l; }
        for (int l = -1; l >= -R; --l) { if (abs(col[8 + l] - col[8 + l + 1]) > 10) break; bwd = -l; }
        const FeReach r = fe_reach(jf, jb, R);
        CHECK(r.fwd == fwd && r.bwd == bwd, "reach: jumps %u %u radius %d: %d %d want %d %d", jf, jb, R, r.fwd, r.bwd, fwd, bwd);
        unsigned window = 0;   // the same backward jumps in point order: bit 4 next to the pick
        for (int l = 0; l < 5; ++l) window |= ((jb >> l) & 1u) << (4 - l);
        CHECK(fe_reach_bwd_window(window, R) == bwd && fe_reach_one(jf, R) == fwd, "reach from a window of jump bits: %u radius %d", window, R);
      }
  return n;
}

// ---- label / continuation by pick count (:196-210, :245-251) ----
static long long labels() {
  long long n = 0;
  for (int nls = 0; nls <= 4; ++nls)
    for (int ns = 0; ns <= nls; ++ns)
      for (int nf = 1; nf <= 4; ++nf) {
        bool ended = false;
        for (int p = 1; p <= 8; ++p, ++n) {
          int lab; bool spread, more;
          fe_pick_label<false>(ns, nls, nf, p, INT_MAX, lab, spread, more);   // the reference: the pick behind the last labelled one is marked, not labelled, and ends the loop
          const int want = p <= ns ? 2 : (p <= nls ? 1 : 0);
          CHECK(lab == want && spread == (want != 0) && more == (want != 0), "sharp pick %d of (%d, %d): label %d spread %d more %d", p, ns, nls, lab, spread, more);
          if (!ended && !more) { CHECK(p == nls + 1 && lab == 0 && !spread, "the loop ends with the unlabelled pick %d, not %d", nls + 1, p); ended = true; }
          int lab2; bool spread2, more2;
          fe_pick_label<false>(ns, nls, nf, p, std::max(ns, nls), lab2, spread2, more2);   // a path that leaves that pick out stops one earlier
          CHECK(lab2 == lab && spread2 == spread && more2 == (want != 0 && p < nls), "sharp pick %d of (%d, %d) with nmax: more %d", p, ns, nls, more2);
          fe_pick_label<true>(ns, nls, nf, p, INT_MAX, lab, spread, more);
          CHECK(lab == -1 && more == (p < nf) && spread == (p < nf), "flat pick %d of %d: label %d spread %d more %d (the n_flat-th ends the loop before the suppression)", p, nf, lab, spread, more);
        }
        CHECK(ended, "the sharp loop ends within %d picks", nls + 1);
      }
  return n;
}

// ---- the pick itself: greedy best-remaining from the header's rules against sort-then-scan (:172-285) ----
struct Ring {
  int M, S, E;                       // points of the cloud, ring_start, ring_end (5 margin points either side of [S, E])
  std::vector<float> cd;             // curvature sums
  std::vector<int> col;
  std::vector<uint8_t> ground, picked0;
};
struct Picks {
  std::vector<int> sharp, less_sharp, flat, less_flat, label;
  std::vector<uint8_t> picked;
  bool operator==(const Picks& o) const { return sharp == o.sharp && less_sharp == o.less_sharp && flat == o.flat && less_flat == o.less_flat && label == o.label && picked == o.picked; }
};
struct PickParams { int formula, nsec, n_sharp, n_less_sharp, n_flat, radius, col_diff; double edge, surf; };

static Picks reference_picks(const Ring& r, const PickParams& P, int* n_ties, int* n_cut, int* n_flat_stop) {
  Picks o;
  o.label.assign(r.M, 0); o.picked = r.picked0;
  std::vector<double> curv(r.M);
  std::vector<int> idx(r.M);
  for (int i = 0; i < r.M; ++i) { curv[i] = (double)r.cd[i] * (double)r.cd[i]; idx[i] = i; }
  auto suppress = [&](int c) {
    for (int l = 1; l <= P.radius; ++l) { if (abs(r.col[c + l] - r.col[c + l - 1]) > P.col_diff) { ++*n_cut; break; } o.picked[c + l] = 1; }
    for (int l = -1; l >= -P.radius; --l) { if (abs(r.col[c + l] - r.col[c + l + 1]) > P.col_diff) { ++*n_cut; break; } o.picked[c + l] = 1; }
  };
  for (int j = 0; j < P.nsec; ++j) {
    int sp, ep;
    if (P.formula == 0) { sp = (r.S * (P.nsec - j) + r.E * j) / P.nsec; ep = (r.S * (P.nsec - 1 - j) + r.E * (j + 1)) / P.nsec - 1; }
    else { sp = r.S + j * (r.E - r.S) / P.nsec; ep = r.S + (j + 1) * (r.E - r.S) / P.nsec - 1; }
    if (sp >= ep) continue;
    // sort_mode 0: the total order (curvature, index)
    std::stable_sort(idx.begin() + sp, idx.begin() + ep + 1, [&](int a, int b) { return curv[a] < curv[b]; });
    for (int k = sp; k < ep; ++k) if (curv[idx[k]] == curv[idx[k + 1]]) ++*n_ties;
    int picked_num = 0;
    for (int k = ep; k >= sp; --k) {
      const int c = idx[k];
      if (o.picked[c] == 0 && curv[c] > P.edge && !r.ground[c]) {
        ++picked_num;
        o.picked[c] = 1;
        if (picked_num <= P.n_sharp) { o.label[c] = 2; o.sharp.push_back(c); o.less_sharp.push_back(c); }
        else if (picked_num <= P.n_less_sharp) { o.label[c] = 1; o.less_sharp.push_back(c); }
        else break;
        suppress(c);
      }
    }
    picked_num = 0;
    for (int k = sp; k <= ep; ++k) {
      const int c = idx[k];
      if (o.picked[c] == 0 && curv[c] < P.surf && r.ground[c]) {
        o.label[c] = -1; o.flat.push_back(c);
        ++picked_num;
        o.picked[c] = 1;
        if (picked_num >= P.n_flat) { ++*n_flat_stop; break; }
        suppress(c);
      }
    }
    for (int k = sp; k <= ep; ++k) if (o.label[k] <= 0) o.less_flat.push_back(k);
  }
  return o;
}

template <bool FLAT>
static void greedy_sector(const Ring& r, const PickParams& P, int sp, int ep, Picks& o) {
  int picked = 0;
  while (true) {
    uint32_t best = fe_key_none<FLAT>();
    int c = -1;
    for (int i = sp; i <= ep; ++i) {   // ascending index: fe_scan_takes decides ties
      const double curv = fe_curvature(r.cd[i]);
      const bool cand = FLAT ? fe_flat_candidate(o.picked[i] != 0, r.ground[i] != 0, fe_curv_surf(curv, P.surf)) : fe_sharp_candidate(o.picked[i] != 0, r.ground[i] != 0, fe_curv_edge(curv, P.edge));
      if (!cand) continue;
      const uint32_t k = fe_curv_key(r.cd[i]);
      if (c < 0 || fe_scan_takes<FLAT>(k, best)) {
        if (c >= 0 && k == best) CHECK(fe_tie_takes<FLAT>(i, c), "fe_scan_takes and fe_tie_takes agree on a tie");
        best = k; c = i;
      }
    }
    if (c < 0) break;
    ++picked;
    int lab; bool spread, more;
    fe_pick_label<FLAT>(P.n_sharp, P.n_less_sharp, P.n_flat, picked, INT_MAX, lab, spread, more);
    o.picked[c] = 1;
    if (lab) o.label[c] = lab;
    if (FLAT) o.flat.push_back(c);
    else { if (lab == 2) o.sharp.push_back(c); if (lab) o.less_sharp.push_back(c); }
    if (spread) {
      unsigned jf = 0, jb = 0;
      for (int l = 0; l < 5; ++l) {
        if (fe_col_jump(r.col[c + l], r.col[c + l + 1], P.col_diff)) jf |= 1u << l;
        if (fe_col_jump(r.col[c - l - 1], r.col[c - l], P.col_diff)) jb |= 1u << l;
      }
      const FeReach reach = fe_reach(jf, jb, P.radius);
      for (int i = c - reach.bwd; i <= c + reach.fwd; ++i) o.picked[i] = 1;
    }
    if (!more) break;
  }
}
static Picks greedy_picks(const Ring& r, const PickParams& P) {
  Picks o;
  o.label.assign(r.M, 0); o.picked = r.picked0;
  for (int j = 0; j < P.nsec; ++j) {
    int sp, ep;
    fe_sector(P.formula, P.nsec, r.S, r.E, j, sp, ep);
    if (fe_sector_skipped(sp, ep)) continue;
    greedy_sector<false>(r, P, sp, ep, o);
    greedy_sector<true>(r, P, sp, ep, o);
    for (int k = sp; k <= ep; ++k) if (fe_less_flat_member(o.label[k])) o.less_flat.push_back(k);
  }
  return o;
}
static long long pick_loops() {
  long long n = 0;
  int ties = 0, cuts = 0, flat_stops = 0, sharp_total = 0, unlabelled = 0;
  for (int it = 0; it < 6000; ++it, ++n) {
    Ring r;
    const int len = rnd(41);   // E - S: rings of up to 40 sector points
    r.M = len + 11 + 6; r.S = 8; r.E = r.S + len;   // (three points more in front of the margin: the cloud does not begin with the ring)
    r.cd.resize(r.M); r.col.resize(r.M); r.ground.resize(r.M); r.picked0.resize(r.M);
    const int nval = 2 + rnd(5);   // few distinct curvature sums: many ties
    int col = rnd(100);
    for (int i = 0; i < r.M; ++i) {
      const float v[] = {0.0f, 0.05f, 0.3f, 0.31f, 0.35f, 1.5f, 4.0f};
      r.cd[i] = v[rnd(nval + 1)] * (rnd(2) ? 1.f : -1.f);   // (+-: the key is |cd|)
      col += rnd(6) ? 1 : 5 + rnd(12);
      r.col[i] = col;
      r.ground[i] = rnd(3) != 0 ? (uint8_t)rnd(2) : (i ? r.ground[i - 1] : (uint8_t)0);
      r.picked0[i] = rnd(7) ? 0 : 1;
    }
    PickParams P;
    P.formula = rnd(2); P.nsec = 1 + rnd(4);
    P.n_less_sharp = rnd(5); P.n_sharp = rnd(P.n_less_sharp + 1); P.n_flat = 1 + rnd(4);
    P.radius = rnd(6); P.col_diff = 10; P.edge = 0.1; P.surf = 0.1;
    int t = 0, c = 0, f = 0;
    const Picks want = reference_picks(r, P, &t, &c, &f), got = greedy_picks(r, P);
    ties += t; cuts += c; flat_stops += f; sharp_total += (int)want.less_sharp.size();
    for (int i = 0; i < r.M; ++i) unlabelled += want.picked[i] && !r.picked0[i] && want.label[i] == 0 && !r.ground[i] ? 1 : 0;
    CHECK(got == want, "ring %d (len %d, %d sectors formula %d, %d/%d/%d, radius %d): %zu/%zu/%zu/%zu picks, want %zu/%zu/%zu/%zu", it, len, P.nsec, P.formula, P.n_sharp,
          P.n_less_sharp, P.n_flat, P.radius, got.sharp.size(), got.less_sharp.size(), got.flat.size(), got.less_flat.size(), want.sharp.size(), want.less_sharp.size(),
          want.flat.size(), want.less_flat.size());
  }
  CHECK(ties > 10000 && cuts > 1000 && flat_stops > 500 && sharp_total > 1000 && unlabelled > 500, "the rings hold what they were drawn for: %d ties, %d cuts, %d flat stops, %d picks, %d",
        ties, cuts, flat_stops, sharp_total, unlabelled);
  // sort_mode 2: of equal curvatures sharp takes the later position of the arrangement, flat the earlier, and the codes order that way
  for (int a = 0; a < 50; ++a)
    for (int b = 0; b < 50; ++b) {
      if (a == b) continue;
      CHECK(fe_tie_takes_arranged<false>(a, b) == (a > b) && fe_tie_takes_arranged<true>(a, b) == (a < b), "arranged ties");
      const uint32_t la = (uint32_t)rnd(768), lb = (uint32_t)rnd(768);
      CHECK((fe_arranged_code<false>(a, la) > fe_arranged_code<false>(b, lb)) == fe_tie_takes_arranged<false>(a, b), "sharp codes: the largest is the later position");
      CHECK((fe_arranged_code<true>(a, la) < fe_arranged_code<true>(b, lb)) == fe_tie_takes_arranged<true>(a, b), "flat codes: the smallest is the earlier position");
      CHECK(fe_arranged_code<false>(a, la) > fe_key_none<false>() && fe_arranged_code<true>(a, la) < fe_key_none<true>() && (fe_arranged_code<false>(a, la) & 0xFFFFu) == la, "codes beat no candidate and keep the index");
    }
  return n;
}

int main() {
  const long long a = sectors(), b = curvature_and_marks(), c = picked_masks(), d = flags(), e = reach(), f = labels(), g = pick_loops();
  printf("sectors %lld, sums and marks %lld, picked bits %lld, flags %lld, reaches %lld, labels %lld, rings %lld\n", a, b, c, d, e, f, g);
  if (g_fail) { printf("fe_rules FAILED: %d checks\n", g_fail); return 1; }
  printf("fe_rules ok\n");
  return 0;
}
