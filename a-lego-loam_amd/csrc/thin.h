// thin.h — host interface of alego_map_thin's kernels (kernels_thin.hip), called by lm_host.hip
#ifndef ALEGO_THIN_H_
#define ALEGO_THIN_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alego_mi355x.h"

struct LmCtx;

// One slot of a thin (or one set of caller arrays, alego_debug_thin_select) as the kernels read it.  The host fills the first part for
// th_select, reads cnt back once and fills the second part: from then on it knows every size.
struct ThJob {
  const float* pose;       // position of frame i at pose[i * pose_stride + 0 .. 2]
  const int* tab;          // the frames' arc_tab rows, or nullptr: no point counts (P' = 0)
  uint8_t* protect;        // [n]; slot >= 0: written by th_select's prologue (frame 0, the resident ring, loop-edge endpoints)
  int* new_id;             // [n] new id of frame i, -1: dropped (the keep mask)
  int* old_id;             // [n] old id of new frame m
  int* new_off;            // [n + 1] new point offset of new frame m; [N'] = P'
  int* cnt;                // [4] N', P', the first dropped id (n: none), the point offset of the rows from there on
  int pose_stride, n, slot;   // slot -1: arrays of the caller
  float r2;                // th_r2(min_dist)
  // ---- after the counts are known
  int n_new, p_new;        // N', P'
  int first;               // the first dropped id: rows and points before it do not move
  int p0;                  // new (= old) point offset of row `first`: points [p0, p_new) move
  int n_loops;
  int stage_pt, stage_row; // where the slot's moved points / rows start in the staging buffers
};
// a moved row on its way through the staging buffer
struct ThRow { int tab[4]; float pose[8]; double stamp; alego_graph_edge e; };

void launch_th_select(const LmCtx& L, ThJob* jobs, int n_jobs, hipStream_t st);
// moved points archive -> stage (items: (job, item of ALEGO_MERGE_COPY_ITEM destination points)), then stage -> archive
void launch_th_gather(const LmCtx& L, const ThJob* jobs, const int2* items, int n_items, float4* stage, hipStream_t st);
void launch_th_scatter(const LmCtx& L, const ThJob* jobs, const int2* items, int n_items, const float4* stage, hipStream_t st);
// moved rows (arc_tab, arc_pose, arc_stamp, pg_chain composed) -> stage; then stage -> rows, the loop edges remapped in place, the counters and the window
void launch_th_rows_read(const LmCtx& L, const ThJob* jobs, int n_jobs, int rows_max, ThRow* stage, hipStream_t st);
void launch_th_rows_write(const LmCtx& L, const ThJob* jobs, int n_jobs, int lanes_max, const ThRow* stage, hipStream_t st);
#endif
