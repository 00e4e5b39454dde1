// api_gate_check.cpp — csrc/api_gate.h against its rules written out plainly (tests/test_api_gate.py builds and runs it with the sanitizers).
// Every case names the expected code and the exact message; a passing list must leave the message string untouched.
#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "api_gate.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const char* const UNTOUCHED = "(untouched)";
static const char* const WHAT = "alego_call";

// ---- the slot-list rule, plainly: walk the list; the first entry outside [0, n_slots) or, with `distinct`, equal to an earlier entry, is the offender
static std::string slot_rule(const std::vector<int>& s, int n_slots, bool distinct) {
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] < 0 || s[i] >= n_slots) return std::string(WHAT) + ": slot out of range";
    if (distinct) for (size_t j = 0; j < i; ++j) if (s[j] == s[i]) return std::string(WHAT) + ": slot " + std::to_string(s[i]) + " is listed twice";
  }
  return UNTOUCHED;
}
static void slot_case(const char* name, const std::vector<int>& s, int n_slots, bool distinct, const std::string& want) {
  CHECK(slot_rule(s, n_slots, distinct) == want, "%s: the plain rule gives '%s', the case expects '%s'", name, slot_rule(s, n_slots, distinct).c_str(), want.c_str());
  std::string err = UNTOUCHED;
  const int rc = gate_slot_list(WHAT, s.empty() ? nullptr : s.data(), (int)s.size(), n_slots, distinct, &err);
  CHECK(rc == (want == UNTOUCHED ? 0 : ALEGO_ERR_ARG), "%s: code %d", name, rc);
  CHECK(err == want, "%s: message '%s', expected '%s'", name, err.c_str(), want.c_str());
}

// ---- the pair-list rule, plainly
static std::string pair_rule(const std::vector<int>& a, const std::vector<int>& b, int n_slots, GatePairs rule) {
  const std::string w(WHAT);
  const size_t n = a.size();
  for (size_t i = 0; i < n; ++i) {
    if (a[i] < 0 || a[i] >= n_slots || b[i] < 0 || b[i] >= n_slots) return w + ": slot out of range";
    if (a[i] == b[i]) return w + ": slot " + std::to_string(a[i]) + " is paired with itself";
    if (rule == GATE_PAIRS_ALIGN) for (size_t j = 0; j < i; ++j) if (a[j] == a[i] && b[j] == b[i]) return w + ": the pair (" + std::to_string(a[i]) + ", " + std::to_string(b[i]) + ") is listed twice";
  }
  if (rule == GATE_PAIRS_MERGE) {
    for (size_t i = 0; i < n; ++i) for (size_t j = 0; j < i; ++j) if (b[j] == b[i]) return w + ": slot " + std::to_string(b[i]) + " is a destination twice";
    for (size_t i = 0; i < n; ++i) for (size_t j = 0; j < n; ++j) if (b[j] == a[i]) return w + ": slot " + std::to_string(a[i]) + " is a destination of one pair and a source of another";
  }
  return UNTOUCHED;
}
static void pair_case(const char* name, const std::vector<int>& a, const std::vector<int>& b, int n_slots, GatePairs rule, const std::string& want) {
  CHECK(pair_rule(a, b, n_slots, rule) == want, "%s: the plain rule gives '%s', the case expects '%s'", name, pair_rule(a, b, n_slots, rule).c_str(), want.c_str());
  std::string err = UNTOUCHED;
  const int rc = gate_pair_list(WHAT, a.empty() ? nullptr : a.data(), b.empty() ? nullptr : b.data(), (int)a.size(), n_slots, rule, &err);
  CHECK(rc == (want == UNTOUCHED ? 0 : ALEGO_ERR_ARG), "%s: code %d", name, rc);
  CHECK(err == want, "%s: message '%s', expected '%s'", name, err.c_str(), want.c_str());
}

int main() {
  const std::string range = "alego_call: slot out of range";
  auto twice = [](int s) { return "alego_call: slot " + std::to_string(s) + " is listed twice"; };
  for (int distinct = 0; distinct < 2; ++distinct) {
    const bool d = distinct != 0;
    slot_case("n = 0 with a null list", {}, 4, d, UNTOUCHED);
    slot_case("n = 0 on a handle of one slot", {}, 1, d, UNTOUCHED);
    slot_case("n_slots = 1, slot 0", {0}, 1, d, UNTOUCHED);
    slot_case("n_slots = 1, slot 1", {1}, 1, d, range);
    slot_case("slot -1", {0, -1}, 4, d, range);
    slot_case("slot n_slots", {4}, 4, d, range);
    slot_case("slot n_slots after valid ones", {3, 2, 4}, 4, d, range);
    slot_case("INT_MIN", {INT_MIN}, 4, d, range);
    slot_case("INT_MAX", {1, INT_MAX}, 4, d, range);
    slot_case("every slot in reverse order", {7, 6, 5, 4, 3, 2, 1, 0}, 8, d, UNTOUCHED);
    slot_case("a duplicate, adjacent", {2, 1, 1, 3}, 4, d, d ? twice(1) : UNTOUCHED);
    slot_case("a duplicate, first and last", {3, 0, 1, 2, 3}, 4, d, d ? twice(3) : UNTOUCHED);
    slot_case("n_slots = 1, slot 0 twice", {0, 0}, 1, d, d ? twice(0) : UNTOUCHED);
    // the first offender in list order is the one named
    slot_case("two duplicates: the one completed first", {0, 1, 1, 0}, 4, d, d ? twice(1) : UNTOUCHED);
    slot_case("a duplicate before a slot out of range", {2, 2, 9}, 4, d, d ? twice(2) : range);
    slot_case("a slot out of range before a duplicate", {9, 2, 2}, 4, d, range);
  }

  for (GatePairs rule : {GATE_PAIRS_ALIGN, GATE_PAIRS_MERGE}) {
    pair_case("n = 0 with null lists", {}, {}, 4, rule, UNTOUCHED);
    pair_case("one pair", {0}, {1}, 2, rule, UNTOUCHED);
    pair_case("a self pair", {0, 2}, {1, 2}, 4, rule, "alego_call: slot 2 is paired with itself");
    pair_case("the source out of range", {4}, {1}, 4, rule, range);
    pair_case("the source negative", {-1}, {1}, 4, rule, range);
    pair_case("the destination out of range", {0, 1}, {1, 4}, 4, rule, range);
    pair_case("the destination INT_MIN", {0}, {INT_MIN}, 4, rule, range);
    pair_case("the source INT_MAX", {INT_MAX}, {0}, 4, rule, range);
    pair_case("a self pair out of range", {7}, {7}, 4, rule, range);
  }
  pair_case("align: (a, b) twice", {0, 2, 0}, {1, 3, 1}, 4, GATE_PAIRS_ALIGN, "alego_call: the pair (0, 1) is listed twice");
  pair_case("align: (a, b) and (b, a) are different pairs", {0, 1}, {1, 0}, 4, GATE_PAIRS_ALIGN, UNTOUCHED);
  pair_case("align: a destination twice and a source twice are legal", {0, 1, 0}, {2, 2, 3}, 4, GATE_PAIRS_ALIGN, UNTOUCHED);
  pair_case("align: a self pair before a repeated pair", {0, 1, 0}, {1, 1, 1}, 4, GATE_PAIRS_ALIGN, "alego_call: slot 1 is paired with itself");
  pair_case("merge: a destination listed twice", {0, 1}, {2, 2}, 4, GATE_PAIRS_MERGE, "alego_call: slot 2 is a destination twice");
  pair_case("merge: (a, b) twice is a destination twice", {0, 0}, {1, 1}, 4, GATE_PAIRS_MERGE, "alego_call: slot 1 is a destination twice");
  pair_case("merge: a destination that is also a source", {0, 1}, {1, 2}, 4, GATE_PAIRS_MERGE, "alego_call: slot 1 is a destination of one pair and a source of another");
  pair_case("merge: (a, b) and (b, a)", {0, 1}, {1, 0}, 4, GATE_PAIRS_MERGE, "alego_call: slot 0 is a destination of one pair and a source of another");
  pair_case("merge: a source listed twice is legal", {0, 0, 0}, {1, 2, 3}, 4, GATE_PAIRS_MERGE, UNTOUCHED);
  pair_case("merge: a destination twice is named before a destination that is a source", {0, 1, 3}, {1, 2, 2}, 4, GATE_PAIRS_MERGE, "alego_call: slot 2 is a destination twice");
  pair_case("merge: a slot out of range in the last pair is named before a destination twice", {0, 1, 9}, {2, 2, 3}, 4, GATE_PAIRS_MERGE, range);

  if (failures) { std::printf("api_gate: %d failure(s)\n", failures); return 1; }
  std::printf("api_gate ok\n");
  return 0;
}
