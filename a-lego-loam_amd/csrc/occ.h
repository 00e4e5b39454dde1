// occ.h — host interface of the occupancy grid's kernels (kernels_occ.hip), called by lm_host.hip
#ifndef ALEGO_OCC_H_
#define ALEGO_OCC_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alego_mi355x.h"
#include "occ_math.h"

struct LmCtx;

#define OCC_T 256             // occ_cast's workgroup = the rays of one work item
#define OCC_PIECE_DEFAULT 32  // steps of a ray one lane walks at a time ("Measured")

// the grid of a handle as the kernels read it
struct OccDev {
  OccGrid G;
  uint32_t *hits, *passes;          // [cells]
  unsigned long long* stats;        // [ALEGO_OCC_STATS] counters of the integrate in flight
};

// items: (frame, chunk of OCC_T selected points of it), frames of `slot`; piece <= 0: one lane per ray
void launch_occ_cast(const LmCtx& L, const OccDev& D, int slot, int kinds, const int2* items, int n_items, int piece, hipStream_t st);
// out[cells], or out[n0 n1] with collapse_z
void launch_occ_classify(const OccDev& D, alego_occ_rule rule, int collapse_z, int8_t* out, hipStream_t st);
void launch_occ_clear(const OccDev& D, hipStream_t st);

// the static map over the same work items, all frames of `slot`
struct OccStatic {
  const int2* items; int n_items;
  const int* frame_off;             // map_offsets' offsets of the frames in assembly order
  int n_pts;                        // selected points = capacity of verdict / pts
  uint8_t* verdict;                 // [n_pts] in assembly order
  float4* pts;                      // [n_pts] the transformed points in assembly order (the assembly scratch)
  int* kept;                        // [n_items] kept points per item
  int* off;                         // [n_items + 1] their exclusive scan
  unsigned long long* stats;        // [ALEGO_STATIC_VERDICTS], zeroed by the launch
};
void launch_occ_mark(const LmCtx& L, const OccDev& D, const OccStatic& S, const alego_static_rule& rule, int slot, int kinds, hipStream_t st);
// the kept points of S.pts, stably, to out[0, out_cap); their number to *n_dev; kinds & ALEGO_MAP_FRAME_ID: w = frame index
void launch_occ_emit(const OccStatic& S, int kinds, float4* out, int out_cap, int* n_dev, hipStream_t st);

// the clearance field (kernels_edt.hip, edt_math.h) of a class array whose domain passed edt_dims_fault
struct EdtWork {
  const int8_t* cls;                // [cells] of the domain n[0] n[1] n[2]
  int32_t n[3];
  int32_t unknown_is_obstacle;
  uint32_t r2;                      // the cap's square; 0: no limit
  uint32_t *a, *b;                  // [cells] each: the passes go back and forth between them
  int2* env; size_t env_cap;        // the envelopes' stacks, [cells] (unused when n[1] = n[2] = 1)
  unsigned long long* stats;        // [ALEGO_EDT_STATS]: sources, FAR cells, the largest finite d2 + 1 (0: none); zeroed by the launch
};
// pass X, passes Y and Z where the axis has more than one cell, the cap and the statistics; returns the one of a / b that holds d2
uint32_t* launch_edt(const EdtWork& W, hipStream_t st);
void launch_edt_cost(const int8_t* cls, const uint32_t* d2, size_t cells, int unknown_is_obstacle, const uint8_t* table, int n_table, int inflate_unknown, uint8_t* out,
                     hipStream_t st);
#endif
