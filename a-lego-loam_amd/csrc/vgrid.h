// vgrid.h — the grid arithmetic of pcl::VoxelGrid<PointXYZI>::applyFilter, shared by every kernel that filters (vox_small,
// fe_voxel, fe_ring_out, gv_*, map_update, lm_total_merge) and by the readers of their bounding boxes.  The grid itself (VGR_FN: getMinMax3D, the
// leaf-too-small rule, geometry, voxel id, voxel key) is also readable by a host compiler without the HIP runtime (tests/vox_merge); the box
// encoding and vgr_bits are device functions only.
#ifndef ALEGO_VGRID_H_
#define ALEGO_VGRID_H_
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VGR_FN __host__ __device__ __forceinline__
#else
#include <math.h>
struct float4 { float x, y, z, w; };
#define VGR_FN static inline
#endif

#if defined(__HIPCC__)
// ---- bounding-box format ----
// A box is 8 words: [0..2] = vgr_enc(min x, y, z), [4..6] = ~vgr_enc(max x, y, z), [3] and [7] unused.  The code preserves
// the order of floats, so atomicMin on every word merges boxes.
__device__ __forceinline__ unsigned vgr_enc(float f) {
  const unsigned b = (unsigned)__float_as_int(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float vgr_dec(unsigned u) { return __int_as_float((int)((u >> 31) ? (u ^ 0x80000000u) : ~u)); }
__device__ __forceinline__ void vgr_box_load(const unsigned* bb, float mn[3], float mx[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) { mn[a] = vgr_dec(bb[a]); mx[a] = vgr_dec(~bb[4 + a]); }
}

#endif

// ---- getMinMax3D ----
// per lane: fminf / fmaxf ignore NaN, as std::min / std::max against a finite running value do
VGR_FN void vgr_box_add(float mn[3], float mx[3], float4 p) {
  mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
  mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
}
// across the wavefront: bfly_minmax_f32 (wave.h), one axis at a time

// ---- the grid ----
// PCL's "leaf size too small" rule: the filter returns its input unchanged
VGR_FN bool vgr_leaf_too_small(const float mn[3], const float mx[3], float inv) {
  const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
  return dx * dy * dz > 2147483647LL;
}

// minb = floor(min * inv), divb = floor(max * inv) - minb + 1, and T = divb[0] divb[1] divb[2] cells.  The rule above bounds
// (max - min) * inv, but divb can exceed it by one per axis, so T can pass 2^32: the voxel id is PCL's int arithmetic, which
// wraps, and is computed here in unsigned (same bits, defined behaviour).
struct VgrGeom {
  int minb[3], divb[3];
  unsigned mul1, mul2;
  unsigned long long T;
};
VGR_FN VgrGeom vgr_geom(const float mn[3], const float mx[3], float inv) {
  VgrGeom g;
#pragma unroll
  for (int a = 0; a < 3; ++a) { g.minb[a] = (int)floorf(mn[a] * inv); g.divb[a] = (int)floorf(mx[a] * inv) - g.minb[a] + 1; }
  g.mul1 = (unsigned)g.divb[0];
  g.mul2 = (unsigned)g.divb[0] * (unsigned)g.divb[1];
  g.T = (unsigned long long)(unsigned)g.divb[0] * (unsigned)g.divb[1] * (unsigned)g.divb[2];
  return g;
}
#if defined(__HIPCC__)
// bits of the u32 voxel id a radix sort has to look at (ids wrap: a grid of 2^32 cells or more needs all 32)
__device__ __forceinline__ int vgr_bits(unsigned long long T) {
  if (T > 0xFFFFFFFFull || T == 0) return 32;
  return T > 1 ? 32 - __clz((int)(unsigned)(T - 1)) : 0;
}
#endif
// integer voxel coordinates of a point relative to the grid (PCL: floor in f32, minus minb as a float)
VGR_FN void vgr_coords(const VgrGeom& g, float4 p, float inv, int* i0, int* i1, int* i2) {
  *i0 = (int)(floorf(p.x * inv) - (float)g.minb[0]);
  *i1 = (int)(floorf(p.y * inv) - (float)g.minb[1]);
  *i2 = (int)(floorf(p.z * inv) - (float)g.minb[2]);
}
VGR_FN unsigned vgr_id(const VgrGeom& g, float4 p, float inv) {   // i0 + i1 mul1 + i2 mul2
  int i0, i1, i2;
  vgr_coords(g, p, inv, &i0, &i1, &i2);
  return (unsigned)i0 + (unsigned)i1 * g.mul1 + (unsigned)i2 * g.mul2;
}

// ---- the bbox-free voxel key of LaserMapping's sorted key frames ----
// PCL's VoxelGrid orders the output by idx = i + j dx + k dx dy with (i, j, k) the integer voxel coordinates relative to the cloud's
// bounding box, i.e. lexicographically by (floor(z inv), floor(y inv), floor(x inv)) — an order that does not depend on the bounding
// box.  21 bits per axis: cells -2^20 .. 2^20 - 1 (419 km at a 0.4 m leaf, 52 km at 0.05).  vkey_pack clamps a cell beyond that range onto the
// last one, which keeps the key well-formed but merges distinct voxels: whoever builds a map by key checks the cloud's box with vkey_holds_box
// first and refuses a cloud that does not fit (map_update: LI_OVERFLOW 8, reported by the host as ALEGO_ERR_CAPACITY).  The key-frame sort needs
// no such check: it orders by box-relative voxel ids, the same order anywhere.
#define VKEY_B (1 << 20)
VGR_FN bool vkey_holds_box(const float mn[3], const float mx[3], float inv) {   // floorf(p * inv) is monotonic in p: the box decides for every point
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (floorf(mn[a] * inv) < -(float)VKEY_B || floorf(mx[a] * inv) > (float)(VKEY_B - 1)) return false;
  return true;
}
VGR_FN int vkey_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }   // (min / max of the HIP runtime: not on a host compiler)
VGR_FN unsigned long long vkey_pack(int ix, int iy, int iz) {
  const int B = VKEY_B;
  const unsigned long long x = (unsigned long long)(unsigned)vkey_clamp(ix + B, 2 * B - 1), y = (unsigned long long)(unsigned)vkey_clamp(iy + B, 2 * B - 1),
                           z = (unsigned long long)(unsigned)vkey_clamp(iz + B, 2 * B - 1);
  return (z << 42) | (y << 21) | x;
}
VGR_FN unsigned long long vkey_of(const float4& p, float inv) {   // floor(p * inverse_leaf_size) as pcl::VoxelGrid computes it (f32)
  return vkey_pack((int)floorf(p.x * inv), (int)floorf(p.y * inv), (int)floorf(p.z * inv));
}

#endif
