// vox_merge.h — the rules of lm_total_merge (kernels_lm.hip): laser_surf_total_ds_ = VoxelGrid(lm_leaf_surf) of laser_surf_ds_ ++ laser_outlier_ds_
// (laserMapping.cpp:337-342) as a stable merge, and VoxelGrid of a cloud of at most LT_OCAP points by counting.  One definition for the kernel and
// for the host check (tests/vox_merge): readable by a host compiler without the HIP runtime, like vgrid.h, whose grid arithmetic it calls.
//
// Why a merge: S = laser_surf_ds_ is the output of VoxelGrid(lm_leaf_surf) a moment earlier, and PCL orders a filter's output by
// (floor(z inv), floor(y inv), floor(x inv)) whatever the bounding box — by the voxel key of vgrid.h.  So S arrives in key order, and the
// stable sort of S ++ O by voxel id, which is all that pcl::VoxelGrid's sort does, is the stable merge of S with the few points of O ordered
// by (key, position).  A centroid may leave its voxel by an ulp (three points at 5.5999994f average to 5.6f, the next 0.8 m cell); that is
// harmless while S stays in order (the run is summed like any other) and is refused when it does not (vm_refuse).
// The sums are PCL's: from 0.f in sorted order, divided by (float)count — a voxel of one point reproduces it, -0.f coming out as +0.f.
#ifndef ALEGO_VOX_MERGE_H_
#define ALEGO_VOX_MERGE_H_
#include "vgrid.h"

#define LT_OCAP 512   // clouds of up to this many points are ordered by counting (an O(n^2 / threads) rank): /outlier of a scan, laser_outlier_ds_ in the merge

typedef unsigned long long vm_u64;

VGR_FN bool vm_finite(const float4& p) { return fabsf(p.x) <= 3.402823466e+38f && fabsf(p.y) <= 3.402823466e+38f && fabsf(p.z) <= 3.402823466e+38f; }

// ---- the stable order of a few keys: rank by counting ----
// position of element i in the stable sort of key[0, n): #{j : key_j < key_i or (key_j == key_i and j < i)}
VGR_FN int vm_rank(const vm_u64* key, int n, int i) {
  const vm_u64 k = key[i];
  int r = 0;
  for (int j = 0; j < n; ++j) r += (key[j] < k || (key[j] == k && j < i)) ? 1 : 0;
  return r;
}

// ---- the stable merge of S (in key order) with O (sorted by (key, position)); S's elements go first among equal keys.  S[i] lands at
// i + #{O keys < its key}, the O element of rank j at j + #{S keys <= its key}: a voxel's run is an S run followed by the O elements of its key ----
// #{sorted keys < key}
VGR_FN int vm_count_less(const vm_u64* sorted, int n, vm_u64 key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
// #{sorted keys <= key}
VGR_FN int vm_count_le(const vm_u64* sorted, int n, vm_u64 key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted[mid] <= key) lo = mid + 1; else hi = mid; }
  return lo;
}

// ---- when the merge does not apply: the general filter (vox_small / vox_big) takes the cloud ----
// sound: no NaN / Inf coordinate, and S's keys are non-decreasing (false after a pass-through first round, or a centroid that left its voxel
// backwards); mn / mx: getMinMax3D of S ++ O.  Inside the key range and with fewer than 2^32 cells the box-relative voxel id of PCL neither wraps nor
// clamps: it is a mixed-radix number of (k, j, i), in the order of the key and equal exactly where the key is.
VGR_FN bool vm_refuse(bool sound, int no, const float mn[3], const float mx[3], float inv) {
  if (!sound || no > LT_OCAP) return true;
  if (!vkey_holds_box(mn, mx, inv) || vgr_leaf_too_small(mn, mx, inv)) return true;
  return vgr_geom(mn, mx, inv).T > 0xFFFFFFFFull;
}

// ---- a voxel's centroid from its run [a, b) of the sorted order; at(j) = the point at sorted position j ----
template <class At>
VGR_FN float4 vm_centroid(At at, int a, int b) {
  float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
  for (int j = a; j < b; ++j) { const float4 p = at(j); sx += p.x; sy += p.y; sz += p.z; si += p.w; }
  const float fn = (float)(b - a);
  float4 c;
  c.x = sx / fn; c.y = sy / fn; c.z = sz / fn; c.w = si / fn;
  return c;
}

#endif
