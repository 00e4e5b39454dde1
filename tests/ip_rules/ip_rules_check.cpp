// ip_rules_check — csrc/ip_rules.h on the host: the row-mask forms of the compaction's decisions equal the per-cell form bit for bit, the per-cell form
// equals the rule of imageProjection.cpp:158-191 written out here as a plain double loop over an image, and the segment rule is right at its thresholds.
// Built with UBSan: no shift of the header leaves its type, whatever ground_scan_id is.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "ip_rules.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static const int kH[] = {1, 4, 5, 6, 9, 10, 11, 64, 70};
static std::vector<int> ground_ids(int NS) { return {-5, -1, 0, 1, NS - 2, NS - 1, NS, NS + 5, INT_MAX}; }

// the rule, from the reference's sweep: a ground cell is kept unless its column is no multiple of 5 and lies more than 4 columns inside either end; an
// active cell of a feasible segment is kept; one of an infeasible segment is an outlier when it lies above ground_scan_id on a column that is a multiple
// of 5, and dropped otherwise; everything else is dropped.  0 drop, 1 keep, 2 outlier.
static int rule(bool ground, bool active, bool feasible, int row, int col, int H, int gsi) {
  if (ground) {
    if (col % 5 != 0 && col > 4 && col < H - 5) return 0;
    return 1;
  }
  if (!active) return 0;
  if (feasible) return 1;
  if (row > gsi && col % 5 == 0) return 2;
  return 0;
}

// per-cell form against the rule: a plain double loop over the image, for every state a cell can be in
static long long cells_against_rule(int NS) {
  long long n = 0;
  for (int H : kH)
    for (int gsi : ground_ids(NS))
      for (int state = 0; state < 4; ++state) {   // empty, ground, active and infeasible, active and feasible
        const bool g = state == 1, a = state >= 2, f = state == 3;
        for (int row = 0; row < NS; ++row)
          for (int col = 0; col < H; ++col) {
            const int want = rule(g, a, f, row, col, H, gsi), got = ip_cell_class(g, a, f, row, col, H, gsi);
            CHECK(got == want, "cell class: NS %d H %d gsi %d state %d row %d col %d: %d, rule %d", NS, H, gsi, state, row, col, got, want);
            ++n;
          }
      }
  return n;
}

// mask forms against the per-cell form for one column state (ground g, active a, feasible cells f) at column col of an image NS x H
template <class M>
static void column(int NS, int H, int col, int gsi, M g, M a, M f) {
  const M above = ip_rows_above<M>(gsi);
  const M keep = ip_col_keep<M>(g, f, col, H), outl = ip_col_outliers<M>(a, f, above, col);
  M wk = 0, wo = 0, wa = 0;
  for (int row = 0; row < NS; ++row) {
    const M bit = (M)1 << row;
    const int c = ip_cell_class((g & bit) != 0, (a & bit) != 0, (f & bit) != 0, row, col, H, gsi);
    if (c == IP_KEEP) wk |= bit;
    if (c == IP_OUTLIER) wo |= bit;
  }
  for (int row = 0; row < IpRowMask<M>::rows; ++row) if (row > gsi) wa |= (M)1 << row;
  CHECK(above == wa, "rows above %d: %llx, want %llx", gsi, (unsigned long long)above, (unsigned long long)wa);
  CHECK(keep == wk && outl == wo, "NS %d H %d col %d gsi %d g %llx a %llx f %llx: keep %llx (cells %llx) outliers %llx (cells %llx)", NS, H, col, gsi,
        (unsigned long long)g, (unsigned long long)a, (unsigned long long)f, (unsigned long long)keep, (unsigned long long)wk, (unsigned long long)outl, (unsigned long long)wo);
}

// NS <= 5: every (ground, active, feasible) triple with ground and active disjoint and feasible within active — four states per row — at every column of
// every H and every ground id.  Larger NS: 10^5 random triples, each at every ground id, at one column; the columns of all H in turn.
template <class M>
static long long masks_against_cells(int NS) {
  long long n = 0;
  const std::vector<int> ids = ground_ids(NS);
  auto triple = [&](uint64_t lo, uint64_t up, M* g, M* a, M* f) {   // two bits per row: rows 0-31 from lo, 32-63 from up
    *g = *a = *f = 0;
    for (int row = 0; row < NS; ++row) {
      const int st = (int)(((row < 32 ? lo : up) >> (2 * (row & 31))) & 3u);   // empty, ground, active and infeasible, active and feasible
      const M bit = (M)1 << row;
      if (st == 1) *g |= bit;
      if (st >= 2) *a |= bit;
      if (st == 3) *f |= bit;
    }
  };
  if (NS <= 5) {
    for (uint64_t code = 0; code < (1ull << (2 * NS)); ++code) {
      M g, a, f;
      triple(code, 0, &g, &a, &f);
      for (int H : kH) for (int col = 0; col < H; ++col) for (int gsi : ids) { column<M>(NS, H, col, gsi, g, a, f); ++n; }
    }
    return n;
  }
  size_t hi = 0;
  int col = 0;
  for (int t = 0; t < 100000; ++t) {
    M g, a, f;
    const uint64_t lo = rnd64(), up = rnd64();
    triple(lo, up, &g, &a, &f);
    CHECK((g & a) == 0 && (f & ~a) == 0, "the test's own triple is not a column state");
    for (int gsi : ids) { column<M>(NS, kH[hi], col, gsi, g, a, f); ++n; }
    if (++col == kH[hi]) { col = 0; hi = (hi + 1) % (sizeof(kH) / sizeof(kH[0])); }
  }
  return n;
}

static void segments() {
  // the defaults: a segment of 30 cells is feasible, one of 5 to 29 when it touches 3 rings
  const int big = 30, vp = 5, vl = 3;
  const struct { int size, rows; bool want; } c[] = {{4, 2, false}, {4, 3, false}, {5, 2, false}, {5, 3, true}, {29, 2, false}, {29, 3, true}, {30, 2, true}, {30, 3, true}};
  for (const auto& k : c) {
    CHECK(ip_seg_feasible(big, vp, vl, k.size, k.rows) == k.want, "segment of %d cells over %d rows: want %d", k.size, k.rows, (int)k.want);
    CHECK(ip_seg_class_feasible(ip_seg_size_class(big, vp, k.size), vl, k.rows) == k.want, "segment of %d cells over %d rows, in two steps: want %d", k.size, k.rows, (int)k.want);
  }
  for (int size = 0; size < 70; ++size)
    for (int rows = 0; rows <= 16; ++rows)
      CHECK(ip_seg_feasible(big, vp, vl, size, rows) == (size >= big || (size >= vp && rows >= vl)), "segment rule at %d cells, %d rows", size, rows);
}

static void numbers() {
  for (int NS : {1, 2, 5, 16, 17, 40, 64})
    for (int gsi : ground_ids(NS))
      for (int row = 0; row < NS; ++row) {
        bool want = false;
        for (int lower = 0; lower < NS - 1 && (long long)lower < (long long)gsi; ++lower) want |= lower + 1 == row;   // :111: the lower cell runs over [0, ground_scan_id)
        CHECK(ip_ground_pair(row, gsi) == want, "ground pair: row %d gsi %d", row, gsi);
      }
  CHECK(ip_root_label(true, 0) == 1 && ip_root_label(true, 41) == 42 && ip_root_label(false, 7) == 0, "root labels");
  CHECK(ip_cell_label(1) == 1 && ip_cell_label(42) == 42 && ip_cell_label(0) == 999999, "cell labels");
  CHECK(ip_ring_start(0) == 5 && ip_ring_start(100) == 105 && ip_ring_end(0) == -6 && ip_ring_end(100) == 94, "ring indices");
  CHECK(ip_intensity(3, 17 / 10000.0) == (float)(3 + 17 / 10000.0) && ip_intensity(0, 0.0) == 0.0f, "intensity");
}

int main() {
  long long cells = 0, cols = 0;
  for (int NS : {1, 2, 5, 16, 17, 40, 64}) cells += cells_against_rule(NS);
  for (int NS : {1, 2, 5, 16}) cols += masks_against_cells<uint32_t>(NS);
  for (int NS : {17, 40, 64}) cols += masks_against_cells<uint64_t>(NS);
  segments();
  numbers();
  printf("%lld cells against the rule, %lld column states against their cells\n", cells, cols);
  if (g_fail) { printf("ip_rules: %d failures\n", g_fail); return 1; }
  printf("ip_rules ok\n");
  return 0;
}
