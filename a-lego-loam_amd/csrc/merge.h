// merge.h — host interface of alego_map_move / alego_map_merge's kernels (kernels_merge.hip), called by lm_host.hip
#ifndef ALEGO_MERGE_H_
#define ALEGO_MERGE_H_
#include <hip/hip_runtime.h>

struct LmCtx;

// one pair of a merge that passed every check, as the kernels read it: the counts are the host's, taken after the initial synchronisation
struct MgPair {
  int src, dst;
  int ns, nd;            // archived frames of the source / of the destination before the merge
  int ps, pd;            // archived points of the source / of the destination before the merge
  int tail;              // min(ns, ring entries): the newest frames of the union that go into the destination's ring
  int pad;
  double T[12];          // dst <- src, row-major 3x4
  double stamp_off;
  double seam_var[6];
};
struct MgMove { int slot, n, pad0, pad1; double T[12]; };   // one slot of a move: its archived frames and the transform

// copy items (pair, item of MG_ITEM points), the per-frame rows and edges, the ring rows of the newest frames
void launch_mg_copy(const LmCtx& L, const MgPair* pairs, const int2* items, int n_items, hipStream_t st);
void launch_mg_frames(const LmCtx& L, const MgPair* pairs, int n_pairs, int ns_max, hipStream_t st);
void launch_mg_ring(const LmCtx& L, const MgPair* pairs, int n_pairs, int tail_max, hipStream_t st);
void launch_mg_move(const LmCtx& L, const MgMove* moves, int n, hipStream_t st);
// lm_store_kf's re-transform of ONE resident frame of every slot of the group with tail[slot] != 0: the j-th oldest of its tail[slot] newest frames
void launch_mg_retransform(const LmCtx& L, const int* tail, int slot0, int n, int j, hipStream_t st);
#endif
