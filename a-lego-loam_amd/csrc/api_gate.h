// api_gate.h — the pure rules of the host API's gate (alego_api.hip): what a list of slots, or of (source, destination) pairs, has to
// satisfy, and the text a refusal carries.  No HIP here: a host compiler reads it alone (tests/api_gate/api_gate_check.cpp).
//
// A gated entry point checks in this order, and the first fault found is the one alego_last_error reports (the code is ALEGO_ERR_ARG either way):
//   1. the handle            null: refused before anything is touched (ALEGO_GATE, alego_api.hip)
//   2. the arguments         a null pointer, a negative count
//   3. the handle's state    what the call needs enabled, and the kind of handle (gate_need, alego_api.hip)
//   4. the options           out of their ranges, not finite; the transforms of alego_map_move / alego_map_merge count as options
//   5. the lists             gate_slot_list / gate_pair_list below: the first offender in list order is named
#ifndef ALEGO_API_GATE_H_
#define ALEGO_API_GATE_H_
#include <algorithm>
#include <cstdint>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/alego_mi355x.h"

// every slot in [0, n_slots) and, with `distinct`, none twice; n == 0 passes whatever `slots` is
inline int gate_slot_list(const char* what, const int32_t* slots, int n, int n_slots, bool distinct, std::string* err) {
  std::vector<char> seen(distinct && n > 0 ? (size_t)std::max(n_slots, 0) : 0, 0);
  for (int i = 0; i < n; ++i) {
    const int s = slots[i];
    if (s < 0 || s >= n_slots) { *err = std::string(what) + ": slot out of range"; return ALEGO_ERR_ARG; }
    if (!distinct) continue;
    if (seen[s]) { *err = std::string(what) + ": slot " + std::to_string(s) + " is listed twice"; return ALEGO_ERR_ARG; }
    seen[s] = 1;
  }
  return 0;
}

// pairs (src[i], dst[i]): both sides in range and different, then
//   GATE_PAIRS_ALIGN   no pair twice; (a, b) and (b, a) are different pairs
//   GATE_PAIRS_MERGE   no destination twice and no destination that is a source of another pair (a source may feed many destinations)
enum GatePairs { GATE_PAIRS_ALIGN, GATE_PAIRS_MERGE };
inline int gate_pair_list(const char* what, const int32_t* src, const int32_t* dst, int n, int n_slots, GatePairs rule, std::string* err) {
  const std::string w(what);
  std::set<std::pair<int, int>> seen;
  for (int i = 0; i < n; ++i) {
    const int a = src[i], b = dst[i];
    if (a < 0 || a >= n_slots || b < 0 || b >= n_slots) { *err = w + ": slot out of range"; return ALEGO_ERR_ARG; }
    if (a == b) { *err = w + ": slot " + std::to_string(a) + " is paired with itself"; return ALEGO_ERR_ARG; }
    if (rule == GATE_PAIRS_ALIGN && !seen.insert({a, b}).second) { *err = w + ": the pair (" + std::to_string(a) + ", " + std::to_string(b) + ") is listed twice"; return ALEGO_ERR_ARG; }
  }
  if (rule != GATE_PAIRS_MERGE || n <= 0) return 0;
  std::vector<char> is_dst((size_t)n_slots, 0);
  for (int i = 0; i < n; ++i) {
    if (is_dst[dst[i]]) { *err = w + ": slot " + std::to_string(dst[i]) + " is a destination twice"; return ALEGO_ERR_ARG; }
    is_dst[dst[i]] = 1;
  }
  for (int i = 0; i < n; ++i)
    if (is_dst[src[i]]) { *err = w + ": slot " + std::to_string(src[i]) + " is a destination of one pair and a source of another"; return ALEGO_ERR_ARG; }
  return 0;
}

#endif
