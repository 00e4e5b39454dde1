// kf_store.h — the layout of the key-frame ring (kf_raw_* / kf_cnt / kf_pose, kfs_*, kf_tmp_*) and of the archive (arc_*, pg_stat) of LmCtx, for kernels
// and host code: no other file indexes kf_cnt, kf_pose, arc_tab, arc_stat or pg_stat with a literal or spells a row out.
#ifndef ALEGO_KF_STORE_H_
#define ALEGO_KF_STORE_H_
#include "../../include/alego_mi355x.h"
#include "lm_ctx.h"
#define KF_FN __host__ __device__ __forceinline__
enum { KF_CORNER = 0, KF_SURF, KF_OUTL, KF_KINDS };   // the clouds of a key frame: column of kf_cnt, position in an archived frame
enum { KF_CNT_W = 4, KF_POSE_W = 8 };                 // ints per row of kf_cnt (points per kind, -); floats per row of kf_pose / arc_pose (x y z roll pitch yaw, 2 unused)
enum { AT_OFF = 0, AT_N = 1, AT_W = 4 };              // arc_tab row: point offset in the slot's arc_pts, then points per kind at AT_N + kind
enum { AS_FRAMES = 0, AS_DROPPED, AS_POINTS, AS_W = 4, PS_LOOPS = 0, PS_CLOSED, PS_EST, PS_W = 4 };   // arc_stat row: frames stored, frames dropped, points stored, -; pg_stat row: loop edges stored, loop_closed_, poses of the last estimate, -
enum { KF_SEL_SURF = 1, KF_SEL_CORNER = 2, KF_SEL_OUTL = 4, KF_SEL_ALL = 7 };   // `kinds` of an assembly (ALEGO_MAP_SURF / _CORNER / _OUTLIER)
// Frame f of slot s is row s * fr_stride + f % fr_mod; kfs_n / kfs_box keep the corner runs (m = 0) of a slot's rows in front of its surf runs
// (m = 1).  *_at and the views take the entry f % fr_mod, which some kernels keep instead of f.
KF_FN int kf_entry(const LmCtx& L, int f) { return f % L.fr_mod; }
KF_FN size_t kf_row_at(const LmCtx& L, int slot, int entry) { return (size_t)slot * L.fr_stride + entry; }
KF_FN size_t kf_row(const LmCtx& L, int slot, int f) { return kf_row_at(L, slot, kf_entry(L, f)); }
KF_FN size_t kf_run_at(const LmCtx& L, int slot, int m, int entry) { return (size_t)slot * 2 * L.fr_stride + (size_t)m * L.fr_mod + entry; }
KF_FN int* kf_cnt_of(const LmCtx& L, size_t row) { return L.kf_cnt + row * KF_CNT_W; }
KF_FN float* kf_pose_of(const LmCtx& L, size_t row) { return L.kf_pose + row * KF_POSE_W; }
KF_FN size_t arc_row(const LmCtx& L, int slot, int f) { return (size_t)slot * L.arc_frames_cap + f; }
KF_FN int* arc_tab_of(const LmCtx& L, int slot, int f) { return L.arc_tab + arc_row(L, slot, f) * AT_W; }
KF_FN float* arc_pose_of(const LmCtx& L, int slot, int f) { return L.arc_pose + arc_row(L, slot, f) * KF_POSE_W; }
KF_FN int* arc_stat_of(const LmCtx& L, int slot) { return L.arc_stat + (size_t)slot * AS_W; }
KF_FN int* pg_stat_of(const LmCtx& L, int slot) { return L.pg_stat + (size_t)slot * PS_W; }
KF_FN int arc_tab_points(const int* tab) { return tab[AT_N + KF_CORNER] + tab[AT_N + KF_SURF] + tab[AT_N + KF_OUTL]; }
// (a selection by kind reads every candidate and picks a VALUE: picking between addresses inside L keeps a copy of L in scratch)
template <class V> KF_FN V kf_pick(int kind, V c, V s, V o) { return kind == KF_CORNER ? c : (kind == KF_SURF ? s : o); }
KF_FN int kf_cap_of(const LmCtx& L, int kind) { return kf_pick(kind, L.kf_cap_c, L.kf_cap_s, L.kf_cap_o); }
KF_FN float4* kf_raw_of(const LmCtx& L, size_t row, int kind) { return kf_pick(kind, L.kf_raw_c, L.kf_raw_s, L.kf_raw_o) + row * kf_cap_of(L, kind); }
// one row of the ring (device pointers): cnt[KF_CNT_W], pose[KF_POSE_W]; raw, cap: the cloud of `kind` and its capacity
struct KfRingRow { size_t row; int* cnt; float* pose; float4* raw; int cap; };
KF_FN KfRingRow kf_ring_row_at(const LmCtx& L, int slot, int entry, int kind) {
  const size_t r = kf_row_at(L, slot, entry);
  return KfRingRow{r, kf_cnt_of(L, r), kf_pose_of(L, r), kf_raw_of(L, r, kind), kf_cap_of(L, kind)};
}
// one archived frame: pts = corner | surf | outlier, pose[KF_POSE_W] (device); from its arc_tab row as the caller can read it (the device's, or a host copy)
struct KfArcFrame { const float4* pts; int nc, ns, no; float* pose; };
KF_FN KfArcFrame kf_arc_frame(const LmCtx& L, int slot, int f, const int* tab) { return KfArcFrame{L.arc_pts + (size_t)slot * L.arc_points_cap + tab[AT_OFF], tab[AT_N + KF_CORNER], tab[AT_N + KF_SURF], tab[AT_N + KF_OUTL], arc_pose_of(L, slot, f)}; }
DEV_INLINE KfArcFrame kf_arc_frame(const LmCtx& L, int slot, int f) { return kf_arc_frame(L, slot, f, arc_tab_of(L, slot, f)); }
// One slot's archive of ANOTHER handle (alego_loc_enable_from_map / _update_from_map: the launch's LmCtx is the localising handle's): plain pointers to the slot's own
// first row of arc_pts / arc_tab / arc_pose and the source's capacities per slot.  A frame or point index beyond them is clamped, never followed.
struct KfArcSrc { const float4* pts; const int* tab; const float* pose; int frames_cap, points_cap; };
inline KfArcSrc kf_arc_src(const LmCtx& L, int slot) { return KfArcSrc{L.arc_pts + (size_t)slot * L.arc_points_cap, arc_tab_of(L, slot, 0), arc_pose_of(L, slot, 0), L.arc_frames_cap, L.arc_points_cap}; }
KF_FN const int* kf_src_tab(const KfArcSrc& S, int f) { return S.tab + (size_t)(f < S.frames_cap ? f : S.frames_cap - 1) * AT_W; }
KF_FN const float* kf_src_pose(const KfArcSrc& S, int f) { return S.pose + (size_t)(f < S.frames_cap ? f : S.frames_cap - 1) * KF_POSE_W; }
KF_FN size_t kf_src_point(const KfArcSrc& S, long long i) { return (size_t)(i < 0 ? 0 : (i < S.points_cap ? i : S.points_cap - 1)); }
// the device words of one frame of a chunk of the batched store build (loc_fill writes them, the frame's two sort jobs read them): points of the corner and of the
// surf + outlier staging run, the store row the sorted runs go to (VoxJob::out_sel), the jobs' enable flag, the counts the jobs write back
enum { LJ_N_C = 0, LJ_N_S, LJ_ROW, LJ_ENABLE, LJ_SORT_N, LJ_SORT_N1, LJ_W = 8 };
// a key frame handed in by the host: no negative count, no missing cloud
inline bool kf_in_valid(const alego_kf_in& k) { return k.n_corner >= 0 && k.n_surf >= 0 && k.n_outlier >= 0 && (!k.n_corner || k.corner) && (!k.n_surf || k.surf) && (!k.n_outlier || k.outlier); }
// A frame is read out as surf, corner, outlier (laserMapping.cpp:607-612, :794-796), restricted to `kinds`: the points that gives, where cloud `kind`
// starts in that order, and output index i -> index in the archive's corner | surf | outlier
KF_FN int kf_sel_count(const KfArcFrame& A, int kinds) { return ((kinds & KF_SEL_CORNER) ? A.nc : 0) + ((kinds & KF_SEL_SURF) ? A.ns : 0) + ((kinds & KF_SEL_OUTL) ? A.no : 0); }
KF_FN int kf_out_start(int nc, int ns, int kinds, int kind) { return kind == KF_SURF ? 0 : ((kinds & KF_SEL_SURF) ? ns : 0) + (kind == KF_CORNER || !(kinds & KF_SEL_CORNER) ? 0 : nc); }
KF_FN int kf_arc_index(int nc, int ns, int kinds, int i) {
  const int c0 = kf_out_start(nc, ns, kinds, KF_CORNER), o0 = kf_out_start(nc, ns, kinds, KF_OUTL);
  return i < c0 ? nc + i : (i < o0 ? i - c0 : nc + ns + (i - o0));
}
// One view of a frame's clouds, whichever store holds it: (pointer, points) per kind in kind order, counted as every reader counts them.
// (built with `kind` a constant after unrolling, so kf_pick selects values and no copy of L goes to scratch)
struct KfClouds { const float4* pts[KF_KINDS]; int n[KF_KINDS]; };
KF_FN int kf_clouds_points(const KfClouds& C) { return C.n[KF_CORNER] + C.n[KF_SURF] + C.n[KF_OUTL]; }
KF_FN KfClouds kf_clouds(const KfArcFrame& A) { return KfClouds{{A.pts, A.pts + A.nc, A.pts + A.nc + A.ns}, {A.nc, A.ns, A.no}}; }
// a row of the ring or the map store, each count clamped to its capacity; cnt: the row's kf_cnt as the caller can read it (the device's, or a host copy)
KF_FN KfClouds kf_clouds_row_at(const LmCtx& L, int slot, int entry, const int* cnt) {
  const size_t r = kf_row_at(L, slot, entry);
  KfClouds C;
#pragma unroll
  for (int k = 0; k < KF_KINDS; ++k) { const int cap = kf_cap_of(L, k); C.pts[k] = kf_raw_of(L, r, k); C.n[k] = cnt[k] < cap ? cnt[k] : cap; }
  return C;
}
DEV_INLINE KfClouds kf_clouds_row_at(const LmCtx& L, int slot, int entry) { return kf_clouds_row_at(L, slot, entry, kf_cnt_of(L, kf_row_at(L, slot, entry))); }
// a slot's current scan (laser_corner_ds_, laser_surf_ds_, laser_outlier_ds_), each count clamped to the capacity of its cloud
static_assert(LI_NCUR_S == LI_NCUR_C + KF_SURF && LI_NCUR_O == LI_NCUR_C + KF_OUTL, "kf_clouds_cur indexes the current scan's counts by kind");
DEV_INLINE KfClouds kf_clouds_cur(const LmCtx& L, int slot) {
  const int* li = L.li + (size_t)slot * LI_COUNT;
  KfClouds C;
#pragma unroll
  for (int k = 0; k < KF_KINDS; ++k) { const int cap = kf_cap_of(L, k); C.pts[k] = kf_pick(k, L.cur_corner_ds, L.cur_surf_ds, L.cur_outl_ds) + (size_t)slot * cap; C.n[k] = min(li[LI_NCUR_C + k], cap); }
  return C;
}
// the frame under m in read-out order (surf, corner, outlier: see kf_sel_count) -> out[0 .. kf_clouds_points(C)); one workgroup of T threads
template <int T> DEV_INLINE void kf_clouds_write(const KfClouds& C, const float m[3][4], float4* out) {
  const int order[KF_KINDS] = {KF_SURF, KF_CORNER, KF_OUTL};
#pragma unroll
  for (int o = 0; o < KF_KINDS; ++o) {
    const float4* pts = C.pts[order[o]];
    const int n = C.n[order[o]];
    for (int i = threadIdx.x; i < n; i += T) out[i] = kf_transform(m, pts[i]);
    out += n;
  }
}
// The body of lm_store_kf (kernels_lm.hip: described there) and pg_retransform; grid (x, 3 kinds, .), T threads.  fresh: the slot's current scan is stored into the row first.
template <int T> DEV_INLINE void kf_row_to_tmp(const LmCtx& L, int slot, int entry, int kind, bool fresh) {
  int* li = L.li + (size_t)slot * LI_COUNT;
  const KfRingRow R = kf_ring_row_at(L, slot, entry, kind);
  float m[3][4];
  keypose_matrix(R.pose, m);
  const float4* cur = kf_pick(kind, L.cur_corner_ds, L.cur_surf_ds, L.cur_outl_ds) + (size_t)slot * R.cap;
  const int n_c = fresh ? min(li[LI_NCUR_C], L.kf_cap_c) : R.cnt[KF_CORNER];
  const int n_s = fresh ? min(li[LI_NCUR_S], L.kf_cap_s) : R.cnt[KF_SURF];
  const int n_o = fresh ? min(li[LI_NCUR_O], L.kf_cap_o) : R.cnt[KF_OUTL];   // (new frame: the current scan's counts; re-transform: the stored ones)
  const int n = min(kf_pick(kind, n_c, n_s, n_o), R.cap);
  float4* dst = kf_pick(kind, L.kf_tmp_c + (size_t)slot * L.kf_cap_c, L.kf_tmp_s + (size_t)slot * L.total_cap, L.kf_tmp_s + (size_t)slot * L.total_cap + n_s);
  for (int i = blockIdx.x * T + threadIdx.x; i < n; i += gridDim.x * T) {
    float4 p;
    if (fresh) { p = cur[i]; R.raw[i] = p; } else { p = R.raw[i]; }
    dst[i] = kf_transform(m, p);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (fresh) R.cnt[kind] = n;
    if (kind == KF_CORNER) { li[LI_TMPN_C] = n_c; li[LI_TMPN_S] = n_s + n_o; li[LI_KF_PEND_RING] = entry; li[LI_KF_PENDING] = 1; }
  }
}
// recent_*_keyframes_.clear() (laserMapping.cpp:563-565; the next mapping frame refills the window, :208-223): set(word of li, value), a kernel stores, the host copies
template <class F> KF_FN void kf_reset_window(F set) { set(LI_REC_CNT, 0); set(LI_DIRTY, 1); set(LI_UVALID, 0); }
#endif
