// Stand-alone check of the two rules of csrc/reloc_math.h that every ICP attempt shares between device and host (tests/test_attempt_math.py builds it
// with -fsanitize=address,undefined and runs it): the candidate word and the attempt window, against values written out here.
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "reloc_math.h"

namespace {
int checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
struct Cand { uint32_t dist, id, shift; };
struct Win { int closest, search_num, last, jlo, jhi; };
}  // namespace

int main() {
  // (a) the candidate word: the corners of (dist <= 20 * 15300, id < 2^24, shift < 60) and a few values between
  CHECK(rl_cand_pack(0, 0, 0) == 0x0ull);
  CHECK(rl_cand_pack(306000, 0xffffff, 59) == 0x0004AB50FFFFFF3Bull);
  CHECK(rl_cand_pack(1, 0, 0) == 0x100000000ull && rl_cand_pack(0, 1, 0) == 0x100ull && rl_cand_pack(0, 0, 1) == 0x1ull);
  std::vector<Cand> all;
  for (uint32_t d : {0u, 1u, 4321u, 305999u, 306000u})
    for (uint32_t i : {0u, 1u, 255u, 256u, 70000u, 0xfffffeu, 0xffffffu})
      for (uint32_t s : {0u, 1u, 31u, 58u, 59u}) all.push_back(Cand{d, i, s});
  for (const Cand& a : all) {
    const unsigned long long c = rl_cand_pack(a.dist, a.id, a.shift);
    CHECK(rl_cand_dist(c) == (int32_t)a.dist && rl_cand_id(c) == (int32_t)a.id && rl_cand_shift(c) == (int32_t)a.shift);
    CHECK(c < RL_CAND_NONE);   // "none" is above every candidate
    for (const Cand& b : all)   // order by `<` is order by (dist, id, shift)
      CHECK((c < rl_cand_pack(b.dist, b.id, b.shift)) == (std::make_tuple(a.dist, a.id, a.shift) < std::make_tuple(b.dist, b.id, b.shift)));
  }
  // a row of words -> ids / dists / shifts; "none" writes nothing
  const unsigned long long row[3] = {rl_cand_pack(7, 3, 59), RL_CAND_NONE, rl_cand_pack(306000, 0xffffff, 0)};
  int32_t ids[3] = {-5, -5, -5}, dists[3] = {-6, -6, -6}, shifts[3] = {-7, -7, -7};
  CHECK(rl_cand_unpack(row, 0, ids, dists, shifts) && !rl_cand_unpack(row, 1, ids, dists, shifts) && rl_cand_unpack(row, 2, ids, dists, shifts));
  CHECK(ids[0] == 3 && dists[0] == 7 && shifts[0] == 59 && ids[1] == -5 && dists[1] == -6 && shifts[1] == -7 && ids[2] == 0xffffff && dists[2] == 306000 && shifts[2] == 0);
  // (b) the attempt window
  const Win wins[] = {
      {0, 25, 98, 0, 25},       // closest = 0: clipped below
      {98, 25, 98, 73, 98},     // closest = last: clipped above
      {40, 25, 98, 15, 65},     // neither
      {40, 0, 98, 40, 40},      // search_num = 0: the candidate alone
      {0, 0, 0, 0, 0},
      {40, 1000, 98, 0, 98},    // search_num larger than the archive: all of it
      {3, 25, 5, 0, 5},
      {0, 25, -1, 0, -1},       // last = -1: no admissible frame, an empty window
      {0, 0, -1, 0, -1},
  };
  for (const Win& w : wins) {
    int jlo = 12345, jhi = 12345;
    lc_window(w.closest, w.search_num, w.last, &jlo, &jhi);
    CHECK(jlo == w.jlo && jhi == w.jhi);
    CHECK((w.last < 0) == (jhi < jlo));
  }
  std::printf("attempt_math ok: %d checks\n", checks);
  return 0;
}
