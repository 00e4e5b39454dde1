// fe_store.h — the layout of DevCtx's structured per-slot arrays (the buffers through which ImageProjection, feature extraction, LaserOdometry and LaserMapping
// hand a scan to one another and the host reads results back), for kernels and host code: no other file indexes one of these arrays, spells a slot, buffer, plane or row stride or a named column out
// or multiplies by SC_COUNT, LO_STATE_N or ALEGO_IMU_Q.  Included by dev_common.h below DevCtx.  Every accessor returns the row its arguments name; an index
// keeps the type of the call site (int where it multiplies in int, size_t else); fe_store_alloc at the end holds the elements per slot of each array.
#ifndef ALEGO_FE_STORE_H_
#define ALEGO_FE_STORE_H_
#define FE_FN __host__ __device__ __forceinline__

// per-slot integer scalars (DevCtx::scal, stride SC_COUNT)
enum {
  SC_FIRST = 0,   // smallest index of a valid input point (orientation, imageProjection.cpp:62)
  SC_LAST,        // largest index of a valid input point
  SC_PVALID,      // valid input points
  SC_M,           // segmented cloud size
  SC_NOUT,        // outlier cloud size
  SC_NFEAS,       // feasible segments (label_cnt_-1)
  SC_LO_INIT,     // system_initialized_ (laserOdometry.cpp:36)
  SC_LO_NSURF,    // surf correspondences of the last scan
  SC_LO_NCORNER,  // corner correspondences
  SC_LO_FLAGS,    // ALEGO_FLAG_* of the last LO step
  SC_LO_ITERS,    // packed solver summaries (surf: it | succ<<8 | term<<16 ; corner <<... in next)
  SC_LO_ITERS2,
  SC_CUR,         // feature double-buffer index holding the features of the last COMPLETED LO step;
                  // FE/LO of the scan in flight write/read buffer SC_CUR^1, lo_solve(phase 1) flips it
  SC_ODOM_VALID,
  SC_LM_FRAME,    // LaserMapping frame_cnt (laserMapping.cpp:111)
  SC_LM_FLAGS,
  SC_PVALID_OUT,  // valid input points of the last projected scan (SC_PVALID is an accumulator, cleared by ip_front)
  SC_FE_EPOCH,    // feature-extraction launches of this slot so far (fe_front increments it; tags the ring counts fe_ring_out's workgroups publish to each other)
  SC_FE_ERR,      // != 0: a workgroup of fe_ring_out gave up waiting for the counts of the rings below it; the slot's less_flat cloud is then treated as EMPTY by
                  // everything that reads it (lo_grid_build, lo_assoc, lm_stage) and the host gets ALEGO_ERR_HIP (fetch_pose).  Sticky until the host clears it
                  // with alego_debug_set_option("ALEGO_FE_ERR_CLEAR", slot) (-1: every slot) — a slot that gave up once keeps failing loudly, never silently
  SC_FE_TICKET,   // fe_ring_out: rings of this launch handed out so far (a workgroup's ring = its ticket, so the rings it waits for belong to workgroups that
                  // are already running whatever order the dispatchers place them in; fe_pickc resets it)
  SC_M_DSK,       // points lo_deskew wrote into seg_dsk (/undistorted): its own count, because ImageProjection of the NEXT scan may rewrite SC_M before a host fetches the cloud
  SC_COUNT = 32
};
#define ALEGO_IMU_Q 200   // imu_queue_length, utility.h:70
enum {
  LS_PARAMS = 0,        // params_[6]
  LS_TW = 6,            // t_w_cur_[3]
  LS_RW = 9,            // r_w_cur_[9] row-major
  LS_PARAMS_SURF = 18,  // params_ after the surf solve (debug)
  LS_COSTS = 24,        // initial/final cost of both solves
  LS_ROT = 32,          // rotation matrix of params_ (row-major), cached for transformToStart ...
  LS_ROT_P = 41,        // ... and the params_ it was computed from (recomputed by lo_assoc when they differ)
  LO_STATE_N = 48
};
// feature cloud kinds: index of feat / fcap, column of feat_cnt; segment of an st_idx row and column of st_cnt (there F_LFLAT is the ring's less_flat_scan)
enum { F_SHARP = 0, F_LSHARP = 1, F_FLAT = 2, F_LFLAT = 3, F_KINDS = 4 };
enum { ST_LFDS = 4, ST_DUMMY = 7, ST_W = 8 };              // st_cnt row: the F_* counts, the ring's less_flat voxels, -, -, a field nothing reads (a harmless target for stores)
enum { RO_LSHARP = 0, RO_LFLAT = 1, RO_PLANES = 2 };       // planes of ring_off / ring_boff
enum { LG_OX = 0, LG_OY, LG_INV_CELL, LG_SETTLE, LG_GX, LG_GY, LG_W = 8 };   // lo_geom row: origin x, y, 1 / cell size, settle threshold, gx, gy (int bits; gx = 0: no grid), -, -
enum { LC_QUERY = 0, LC_CLOSEST = 1, LC_W = 4 };           // lo_corr row: query, closest, idx2, idx3; closest < 0 = none
enum { RC_KEEP = 0, RC_OUT, RC_FEAS, RC_W = 4 };           // row_cnt row: kept cells, outliers, feasible roots, -; the planes of ipb_off are the same three
enum { IPO_ROWS = 64, IPO_PLANES = 3 };
enum { PO_ODOM_T = 0, PO_ODOM_Q = 3, PO_MAP_T = 7, PO_MAP_Q = 10, PO_LOG_W = 14, PO_W = 16 };   // poses row: odom t, q (w x y z), map t, q, -, -; a traj row is its first PO_LOG_W
enum { IMU_TIME = 0, IMU_RPY = 1, IMU_SHIFT = 4, IMU_VELO = 7, IMU_W = 10 };   // imu_ring row (imu_time_ ... imu_velo_z_)
enum { IMP_LAST = 0, IMP_FRONT, IMP_LAST_ITER, IMP_N = 3, IMP_W = 4 };         // imu_ptr row: imu_ptr_last_, imu_ptr_front_, imu_ptr_last_iter_, -
enum { ORI_N = 3, ORI_W = 4 };                             // ori row: start, end, difference of the scan's orientation, -

// ---- a LaserOdometry kind (0 surf, 1 corner): the cloud it matches against, that cloud's plane of ring_off / ring_boff; its box set / grid is `kind` itself ----
FE_FN constexpr int lo_target(int kind) { return kind == 0 ? F_LFLAT : F_LSHARP; }
FE_FN constexpr int lo_plane(int kind) { return kind == 0 ? RO_LFLAT : RO_LSHARP; }
FE_FN constexpr int box_set_of(int k) { return k == F_LFLAT ? 0 : 1; }   // the box set of feature cloud k (F_LFLAT or F_LSHARP)

// ---- image projection ----
// (scal_at, ring_at: the offsets alone, for ip_fused_t, which fetches the array pointers late from the kernel-argument segment)
template <class I> FE_FN I scal_at(I slot) { return slot * SC_COUNT; }
template <class I> FE_FN int* scal_of(const DevCtx& d, I slot) { return d.scal + scal_at(slot); }
FE_FN constexpr size_t scal_n() { return SC_COUNT; }   // (<array>_n: elements per slot, where the host needs one outside fe_store_alloc)
template <class I> FE_FN float* ori_of(const DevCtx& d, I slot) { return d.ori + slot * ORI_W; }
template <class I, class R> FE_FN auto ring_at(int n_rings, I slot, R ring) { return slot * n_rings + ring; }
template <class I, class R> FE_FN int* ring_start_of(const DevCtx& d, I slot, R ring) { return d.ring_start + ring_at(d.NS, slot, ring); }
template <class I, class R> FE_FN int* ring_end_of(const DevCtx& d, I slot, R ring) { return d.ring_end + ring_at(d.NS, slot, ring); }
template <class I, class R> FE_FN int* ring_end_before(const DevCtx& d, I slot, R ring) { return ring_end_of(d, slot, ring) - 1; }   // of ring - 1, closed when `ring` starts (ring = NS: the last)
FE_FN int* row_cnt_of(const DevCtx& d, int slot, int row) { return d.row_cnt + ((size_t)slot * d.NS + row) * RC_W; }
// the banded path (kernels_ipb.hip): mask k of IPB_NM, one 64-bit word of rows per column; plane k of ipb_off from chunk `ch` of `nch` chunks of 64 columns on
FE_FN unsigned long long* ipb_mask(const DevCtx& d, int slot, int k) { return d.ipb_col + ((size_t)slot * IPB_NM + k) * d.H; }
FE_FN size_t ipb_col_n(const DevCtx& d) { return (size_t)IPB_NM * d.H; }
template <int K> FE_FN int* ipb_off_of(const DevCtx& d, int slot, int nch) { return d.ipb_off + ((size_t)slot * IPO_PLANES + K) * IPO_ROWS * nch; }
FE_FN size_t ipb_off_n(const DevCtx& d) { return (size_t)IPO_PLANES * IPO_ROWS * ((d.H + 63) / 64); }

// ---- per-ring staging of feature extraction ----
// (a ring is an int, or a size_t sum where the call site adds in size_t)
// a row of st_idx is sharp | less_sharp | flat | less_flat_scan: p moved to the start of segment `part` (an offset or a pointer), added segment by segment
template <class T> FE_FN T st_seg(const DevCtx& d, T p, int part) { if (part > F_SHARP) p += d.cap_sharp; if (part > F_LSHARP) p += d.cap_lsharp; return part > F_FLAT ? p + d.cap_flat : p; }
FE_FN int st_part(const DevCtx& d, int part) { return st_seg(d, 0, part); }
template <class R> FE_FN int* st_idx_of(const DevCtx& d, int slot, R ring) { return d.st_idx + ((size_t)slot * d.NS + ring) * d.st_stride; }
template <class R> FE_FN int* st_idx_of(const DevCtx& d, int slot, R ring, int part) { return st_seg(d, st_idx_of(d, slot, ring), part); }
template <class R> FE_FN int* st_cnt_of(const DevCtx& d, int slot, R ring) { return d.st_cnt + ((size_t)slot * d.NS + ring) * ST_W; }
template <class R> FE_FN float4* st_lfds_of(const DevCtx& d, int slot, R ring) { return d.st_lfds + ((size_t)slot * d.NS + ring) * d.H; }
// the same row as fe_cand's candidate staging (the fused path never filters into it): 2 H entries per ring
FE_FN uint2* st_cand_of(const DevCtx& d, int slot, int ring) { return reinterpret_cast<uint2*>(st_lfds_of(d, slot, ring)); }
FE_FN unsigned* fe_sync_of(const DevCtx& d, int slot, int ring) { return d.fe_sync + ((size_t)slot * d.NS + ring); }

// ---- feature clouds, double-buffered: fb = fbuf(slot, buffer) ----
FE_FN size_t fbuf(int slot, int buffer) { return (size_t)slot * 2 + buffer; }
// buffer written by the scan in flight (valid from fe_collect until lo_solve phase 1 flips SC_CUR)
FE_FN int cur_in_flight(const DevCtx& d, int slot) { return d.scal[slot * SC_COUNT + SC_CUR] ^ 1; }
// fb of the scan in flight / of the previous scan, as LaserOdometry sees them.  A lane never runs lo_solve, so its SC_CUR stays at its initial 1 and
// feature extraction always fills its buffer 0.
FE_FN size_t fidx_cur(const DevCtx& d, int slot) { return d.fs_cur >= 0 ? (size_t)d.fs_cur * 2 : (size_t)slot * 2 + cur_in_flight(d, slot); }
FE_FN size_t fidx_last(const DevCtx& d, int slot) { return d.fs_last >= 0 ? (size_t)d.fs_last * 2 : (size_t)slot * 2 + (cur_in_flight(d, slot) ^ 1); }
// slot whose per-scan outputs (poses, outlier cloud, outlier count) belong to the scan in flight
FE_FN int scan_slot_of(const DevCtx& d, int slot) { return d.fs_cur >= 0 ? d.fs_cur : slot; }
template <class I> FE_FN float4* feat_of(const DevCtx& d, int k, I fb) { return d.feat[k] + fb * d.fcap[k]; }
template <class I> FE_FN int* feat_idx_of(const DevCtx& d, int k, I fb) { return d.feat_idx[k] + fb * d.fcap[k]; }
template <class I> FE_FN int* feat_cnt_of(const DevCtx& d, I fb) { return d.feat_cnt + fb * F_KINDS; }
template <class I, class P> FE_FN int* ring_off_of(const DevCtx& d, I fb, P plane) { return d.ring_off + (fb * RO_PLANES + plane) * (d.NS + 1); }
template <class I, class P> FE_FN int* ring_boff_of(const DevCtx& d, I fb, P plane) { return d.ring_boff + (fb * RO_PLANES + plane) * (d.NS + 1); }

// ---- laser odometry: targets of (fb, kind) ----
// row of the [slot][2 buffers][2 kinds] arrays: (fb, kind) for lo_cell and lo_geom, (fb, box set) for lo_box.  A caller computes it once and hands it to each
template <class I, class K> FE_FN auto lo_row(I fb, K kind) { return fb * 2 + kind; }
template <class I> FE_FN float4* lo_box_of(const DevCtx& d, I row) { return d.lo_box + row * d.lo_box_cap * 2; }   // box b is the pair [2 b] min, [2 b + 1] max corner: the one width its users write themselves
// the target cloud of a kind and its copy sorted by grid cell (a kind known only at run time picks between two rows, not between two addresses inside d)
template <class I> FE_FN float4* lo_targets_of(const DevCtx& d, int kind, I fb) { return kind == 0 ? feat_of(d, F_LFLAT, fb) : feat_of(d, F_LSHARP, fb); }
template <class I> FE_FN float4* lo_cpts_of(const DevCtx& d, int kind, I fb) { return kind == 0 ? d.lo_cpts[0] + fb * d.fcap[F_LFLAT] : d.lo_cpts[1] + fb * d.fcap[F_LSHARP]; }
template <class I> FE_FN unsigned short* lo_cell_of(const DevCtx& d, I row) { return d.lo_cell + row * (LO_GC + 2); }
template <class I> FE_FN float* lo_geom_of(const DevCtx& d, I row) { return d.lo_geom + row * LG_W; }
// correspondence row q of (slot, kind): the surf rows of a slot, then its corner rows
template <class Q = int> FE_FN int* lo_corr_of(const DevCtx& d, int slot, int kind, Q q = 0) { return d.lo_corr + ((size_t)slot * (d.lo_qcap_surf + d.lo_qcap_corner) + (kind == 0 ? 0 : d.lo_qcap_surf) + q) * LC_W; }
FE_FN double* lo_state_of(const DevCtx& d, int slot) { return d.lo_state + (size_t)slot * LO_STATE_N; }
FE_FN constexpr size_t lo_state_n() { return LO_STATE_N; }
FE_FN double* imu_ring_of(const DevCtx& d, int slot) { return d.imu_ring + (size_t)slot * ALEGO_IMU_Q * IMU_W; }
template <class P> FE_FN P* imu_row(P* ring, int j) { return ring + j * IMU_W; }
FE_FN constexpr size_t imu_ring_n() { return (size_t)ALEGO_IMU_Q * IMU_W; }
FE_FN int* imu_ptr_of(const DevCtx& d, int slot) { return d.imu_ptr + (size_t)slot * IMP_W; }

// ---- outputs ----
FE_FN double* poses_of(const DevCtx& d, int slot) { return d.poses + (size_t)slot * PO_W; }
FE_FN double* traj_of(const DevCtx& d, int slot, int k) { return d.traj + ((size_t)slot * d.traj_cap + k) * PO_LOG_W; }
FE_FN int* traj_n_of(const DevCtx& d, int slot) { return d.traj_n + slot; }

// ---- elements per slot, from the constants the accessors stride by: alego_create takes every array above through alloc(&member, elements, zero-filled), B = n_slots
// (ipb_col / ipb_off exist only for the banded path and stay with their condition: ipb_col_n, ipb_off_n) ----
template <class A> int fe_store_alloc(DevCtx& d, size_t B, A alloc) {
  const size_t NS = d.NS;
  int rc = alloc(&d.scal, B * scal_n(), true);
  rc |= alloc(&d.ori, B * ORI_W, true); rc |= alloc(&d.ring_start, B * NS, true); rc |= alloc(&d.ring_end, B * NS, true); rc |= alloc(&d.row_cnt, B * NS * RC_W, true);
  rc |= alloc(&d.st_idx, B * NS * d.st_stride, true); rc |= alloc(&d.st_cnt, B * NS * ST_W, true); rc |= alloc(&d.st_lfds, B * NS * d.H, true); rc |= alloc(&d.fe_sync, B * NS, true);
  for (int k = 0; k < F_KINDS; ++k) rc |= alloc(&d.feat[k], B * 2 * d.fcap[k], true);
  for (int k = 0; k < F_LFLAT; ++k) rc |= alloc(&d.feat_idx[k], B * 2 * d.fcap[k], true);
  rc |= alloc(&d.feat_cnt, B * 2 * F_KINDS, true); rc |= alloc(&d.ring_off, B * 2 * RO_PLANES * (NS + 1), true); rc |= alloc(&d.ring_boff, B * 2 * RO_PLANES * (NS + 1), true);
  for (int kind = 0; kind < 2; ++kind) rc |= alloc(&d.lo_cpts[kind], B * 2 * d.fcap[lo_target(kind)], false);
  rc |= alloc(&d.lo_box, B * 2 * 2 * d.lo_box_cap * 2, true); rc |= alloc(&d.lo_cell, B * 2 * 2 * (LO_GC + 2), true); rc |= alloc(&d.lo_geom, B * 2 * 2 * LG_W, true);
  rc |= alloc(&d.lo_corr, B * (d.lo_qcap_surf + d.lo_qcap_corner) * LC_W, true); rc |= alloc(&d.lo_state, B * lo_state_n(), true); rc |= alloc(&d.poses, B * PO_W, true);
  rc |= alloc(&d.imu_ring, B * imu_ring_n(), true); rc |= alloc(&d.imu_ptr, B * IMP_W, true);
  return rc;
}
#endif
