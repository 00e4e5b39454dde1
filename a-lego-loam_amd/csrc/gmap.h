// gmap.h — the global map: the device key-frame archive (alego_map_*) and the device-wide pcl::VoxelGrid it is filtered with
// (kernels_gmap.hip).
#ifndef ALEGO_GMAP_H_
#define ALEGO_GMAP_H_
#include <hip/hip_runtime.h>

#include <string>

#include "dev_mem.h"
#include "voxel.h"

struct DevCtx;
struct LmCtx;

// clouds of at most this many points are filtered by one workgroup (vox_small / vox_big, kernels_voxel.hip); larger ones by the
// multi-kernel path below.  Measured in DESIGN.md section 11 (tools/gmap_timing.py); ALEGO_GV_SMALL_MAX overrides.
#ifndef GV_SMALL_MAX_DEFAULT
#define GV_SMALL_MAX_DEFAULT 32768
#endif

// Device-wide VoxelGrid scratch of one handle: sized by the largest cloud it has filtered (grown, never per call)
struct GvCtx {
  int cap = 0;                   // points in / out / sort buffers hold
  int small_max = GV_SMALL_MAX_DEFAULT;
  float4 *in = nullptr, *out = nullptr;
  unsigned *kA = nullptr, *kB = nullptr;     // voxel keys (radix ping-pong)
  int *vA = nullptr, *vB = nullptr;          // point indices (radix ping-pong)
  int* run = nullptr;            // [cap] run flags, then their exclusive scan (output rank of every voxel head)
  int* starts = nullptr;         // [cap + 1] first sorted position of every voxel
  int* hist = nullptr;           // [256][tiles] digit counts per tile, scanned in place
  int* bsum = nullptr;           // block sums of the scans
  unsigned* bbox = nullptr;      // [8] encoded min xyz / ~max xyz
  int* geom = nullptr;           // [16] minb xyz, mul1, mul2, pass-through, radix passes (gv_geom)
  int* cnt = nullptr;            // [2] points in, voxels out
  VoxCtx small;                  // one job over in -> out with capacity small_max (vox_small / vox_big)
  int small_cap = 0;
  DevPool mem;                   // owns every array above
};
int gv_small_max_env();   // GV_SMALL_MAX_DEFAULT, or ALEGO_GV_SMALL_MAX
int gv_reserve(GvCtx* G, int n, std::string* err);
void gv_destroy(GvCtx* G);
// VoxelGrid(leaf) of the n points in G->in (n known to the host, G->cnt[0] = n on the device) into G->out; the voxel count is left in
// G->cnt[1]
int gv_filter(GvCtx* G, int n, float leaf, hipStream_t st, std::string* err);

// the archive (LmCtx::arc_*): append the key frame lm_store_kf just wrote (force = 0: the slots whose LI_KF_ADDED is set; force = 1:
// the newest key frame of every slot of the launch, alego_lm_add_keyframe)
void launch_map_archive(const DevCtx& d, const LmCtx& L, int force, hipStream_t st);
// global map of one slot: selected points of archived frames [0, nf) transformed by their archived poses, concatenated into `out`
// (capacity of the archive's max_points); the point count goes to *n_dev
void launch_map_assemble(const LmCtx& L, int slot, int nf, int kinds, float4* out, int* off_scratch, int* n_dev, hipStream_t st);
// its first half alone: off[f] = selected points of frames [0, f), off[nf] = *n_dev = the total (the static map, kernels_occ.hip)
void launch_map_offsets(const LmCtx& L, int slot, int nf, int kinds, int* off, int* n_dev, hipStream_t st);

#endif
