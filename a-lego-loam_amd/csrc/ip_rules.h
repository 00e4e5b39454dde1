// ip_rules.h — the output rules of ImageProjection, everything behind phase B's two decisions (ip_pred.h): which segment is feasible
// (imageProjection.cpp:282-301), which cell of the image is kept, which is an outlier and how ground is thinned (:158-191), the ring
// indices (:161,:190), the label numbers (:303-314) and a point's intensity (:101).  Five kernel paths produce cloud_info bit for bit
// alike; each of them takes its rules from here, per cell or on a column's row masks.  Plain numbers in, no DevCtx.
// Readable by a host compiler without the HIP runtime: tests/ip_rules/ip_rules_check.cpp compares the mask forms with the per-cell form,
// and that one with the rule written out, on the CPU.
#ifndef ALEGO_IP_RULES_H_
#define ALEGO_IP_RULES_H_
#include <stdint.h>
#include "ip_pred.h"   // IP_PRED_FN

// a segment survives when it is big, or of medium size and spread over enough rings (:282-301)
// In two steps, for the kernels that hold a segment's size and its row mask one after the other in the same 16 bits of LDS: the size says
// "feasible", "never", or "the rows decide".
enum { IP_SEG_SMALL = 0, IP_SEG_MID = 1, IP_SEG_BIG = 2 };
IP_PRED_FN int ip_seg_size_class(int big, int valid_points, int size) { return size >= big ? IP_SEG_BIG : (size >= valid_points ? IP_SEG_MID : IP_SEG_SMALL); }
IP_PRED_FN bool ip_seg_class_feasible(int size_class, int valid_lines, int n_rows) { return size_class == IP_SEG_BIG || (size_class == IP_SEG_MID && n_rows >= valid_lines); }
IP_PRED_FN bool ip_seg_feasible(int big, int valid_points, int valid_lines, int size, int n_rows) {
  return ip_seg_class_feasible(ip_seg_size_class(big, valid_points, size), valid_lines, n_rows);
}
// the pair of cells (row - 1, row) takes the ground test (:111: the lower row runs over [0, ground_scan_id))
IP_PRED_FN bool ip_ground_pair(int row, int ground_scan_id) { return row >= 1 && row - 1 < ground_scan_id; }

// ---- a cell's class in the compaction sweep (:164-188) ----
// ground is thinned to every fifth column away from the image's two ends (:173-176); a cell of an infeasible segment is an outlier
// above the ground rings on every fifth column (:165-171), and dropped elsewhere
enum { IP_DROP = 0, IP_KEEP = 1, IP_OUTLIER = 2 };
IP_PRED_FN bool ip_ground_col_kept(int col, int H) { return col % 5 == 0 || col <= 4 || col >= H - 5; }
IP_PRED_FN bool ip_outlier_col(int col) { return col % 5 == 0; }
IP_PRED_FN int ip_cell_class(bool ground, bool active, bool feasible, int row, int col, int H, int ground_scan_id) {
  if (ground) return ip_ground_col_kept(col, H) ? IP_KEEP : IP_DROP;
  if (!active) return IP_DROP;
  if (feasible) return IP_KEEP;
  return (row > ground_scan_id && ip_outlier_col(col)) ? IP_OUTLIER : IP_DROP;
}

// ---- the same decision on a column's row masks: bit r = row r; M = uint32_t holds 16 rows, uint64_t holds 64 ----
template <class M> struct IpRowMask {
  static_assert(sizeof(M) == 4 || sizeof(M) == 8, "a row mask is a uint32_t (16 rows) or a uint64_t (64 rows)");
  static constexpr int rows = sizeof(M) == 8 ? 64 : 16;
  static constexpr M all = sizeof(M) == 8 ? ~(M)0 : (M)0xFFFFu;
};
// rows > ground_scan_id, for every int: all rows below zero, none from rows - 1 on (no shift count leaves [0, rows - 2])
template <class M> IP_PRED_FN M ip_rows_above(int ground_scan_id) {
  if (ground_scan_id < 0) return IpRowMask<M>::all;
  if (ground_scan_id >= IpRowMask<M>::rows - 1) return (M)0;
  return IpRowMask<M>::all & ~((((M)2) << ground_scan_id) - (M)1);
}
// kept cells of a column: the cells of feasible segments, and its ground where ground is kept
template <class M> IP_PRED_FN M ip_col_keep(M ground, M feasible, int col, int H) { return (ip_ground_col_kept(col, H) ? ground : (M)0) | feasible; }
// outliers of a column; `above` = ip_rows_above(ground_scan_id)
template <class M> IP_PRED_FN M ip_col_outliers(M active, M feasible, M above, int col) { return ip_outlier_col(col) ? (active & ~feasible & above) : (M)0; }

// ---- numbers written out ----
// label_cnt_ numbering (:303-306): the roots of feasible segments count 1, 2, .. in discovery order (rank = feasible roots before this
// one), the root of an infeasible one holds 0; a cell's label is its root's number, 999999 where that is 0 (:307-314)
IP_PRED_FN int ip_root_label(bool feasible, int rank) { return feasible ? rank + 1 : 0; }
IP_PRED_FN int ip_cell_label(int root_label) { return root_label > 0 ? root_label : 999999; }
// startRingIndex / endRingIndex (:161,:190) from the output line of a ring's first kept cell and of the next ring's (the total behind the last)
IP_PRED_FN int ip_ring_start(int first_line) { return first_line + 5; }
IP_PRED_FN int ip_ring_end(int next_first_line) { return next_first_line - 1 - 5; }
// intensity = row + column / 10000 (:101); colfrac = the column's fraction, divided once on the host
IP_PRED_FN float ip_intensity(int row, double colfrac) { return (float)(row + colfrac); }

#endif
