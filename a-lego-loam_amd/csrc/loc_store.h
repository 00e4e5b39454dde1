// loc_store.h — host entry points of the batched build of a localising handle's map store from a slot's archive of a mapping handle
// (alego_loc_enable_from_map / alego_loc_update_from_map; kernels_loc.hip), called by lm_host.hip
#ifndef ALEGO_LOC_STORE_H_
#define ALEGO_LOC_STORE_H_
#include "kf_store.h"

// frames f0 .. f0 + chunk - 1 of S -> rows of the same ids of the store L names (raw clouds, counts, pose) and slots 0 .. chunk - 1 of the staging
// area (stage_c [chunk][kf_cap_c], stage_s [chunk][total_cap]) and of words [chunk][LJ_W]; a slot whose frame is >= n_frames only gets its enable
// word cleared.  n_max: most points of one cloud of the chunk's frames (the host's copy of arc_tab).
void launch_loc_fill(const LmCtx& L, const KfArcSrc& S, int f0, int n_frames, int chunk, int n_max, float4* stage_c, float4* stage_s, int* words, hipStream_t st);
// kf_reset_window for every slot of the handle
void launch_loc_reset_windows(const LmCtx& L, int n_slots, hipStream_t st);
#endif
