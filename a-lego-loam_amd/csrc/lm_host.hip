// lm_host.hip — LaserMapping: HBM allocation and kernel sequencing (no numerics here).
#include "lm_host.h"
#include "api_gate.h"
#include "dev_copy.h"
#include "dev_mem.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

#include <rccl/rccl.h>

#include "kf_store.h"
#include "voxel.h"
#include "vox_merge.h"
#include "gmap.h"
#include "loc_math.h"
#include "pgraph.h"
#include "merge.h"
#include "merge_math.h"
#include "thin.h"
#include "thin_math.h"
#include "edt_math.h"
#include "occ.h"
#include "loc_store.h"
#include "remap_math.h"

struct LmHost {
  alego_params P;
  int n_slots;
  int gsize;                   // slots per stream group
  std::vector<hipStream_t> st; // one HIP stream per group
  LmCtx L;
  // per group — vm: map corner, map surf of every slot (jobs 2 b, 2 b + 1), then scan corner, scan surf, scan outlier of every
  // slot: the filters of the current scan do not depend on the map, so they share the map round's three launches;
  // v2: scan surf_total (needs the first round's outputs)
  std::vector<VoxCtx> vm, v2;
  std::vector<VoxCtx> vk;      // per group: the two key-frame sort jobs of every slot alone (set_keypose / add_keyframe, outside the regular sequence)
  std::vector<MapWork> work;   // per group: work list of map_accum
  std::vector<int> tm_grid1, tm_grid, tm_par;   // per stream group under ALEGO_LM_TOTAL_MERGE: workgroups of round 1's and of round 2's vox_small launch; which set of list counters the next lm_total_merge uses
  bool fallback_ok = true;     // buffers of the concat + radix VoxelGrid path (ALEGO_MAP_MERGE=0) are allocated
  ncclComm_t comm = nullptr;   // alego_dist_init: the registration of every slot is sharded over the ranks of this communicator
  std::string dist_err;
  DevPool mem;               // every device block LaserMapping owns apart from the VoxelGrid contexts and gv
  std::vector<long> frames;  // host mirror of frame_cnt per slot: only used to skip launches
  // the global map (alego_map_* / alego_voxel_grid): device-wide VoxelGrid scratch + the assembly's frame offsets
  GvCtx gv;
  int* arc_off = nullptr;      // [arc_frames_cap + 1]
  // localisation mode (alego_loc_enable): the two sort jobs that fill the map store, frame after frame
  VoxCtx vloc;
  bool vloc_made = false;
  int loc_chunk = 128;         // alego_loc_enable_from_map / _update_from_map: frames per chunk of the batched build (ALEGO_LOC_CHUNK), before the byte budget clamps it
  // alego_map_move / alego_map_merge: the pairs, copy items, per-slot tail words and moves of a call; allocated by the first call and kept
  DevBuf<MgPair> mg_pairs;
  DevBuf<int2> mg_items;
  DevBuf<int> mg_tail;
  DevBuf<MgMove> mg_moves;
  // alego_map_thin / alego_debug_thin_select: the jobs, their id tables and offsets, protect masks, copy items, the staged points and rows of a
  // call, the caller's poses of the debug entry; allocated by the first call and kept
  DevBuf<ThJob> th_jobs;
  DevBuf<int> th_ints;
  DevBuf<uint8_t> th_prot;
  DevBuf<int2> th_items;
  DevBuf<float4> th_pts;
  DevBuf<ThRow> th_rows;
  DevBuf<float> th_pose;
  // alego_regcov_enable: the resolved options (reg_cov_math.h) as the device holds them
  bool rc_on = false;
  double rc_opt[RC_OPT_W] = {};
  // alego_remap_enable
  bool rm_on = false;
  // alego_occ_enable: the grid (hits, passes and the counters of an integrate belong to mem), the options it was made from, the work list of an
  // integrate and the classes of a classify, both allocated by the first call and kept
  bool occ_on = false;
  OccDev occ = {};
  alego_occ_opts occ_opts = {};
  int occ_piece = OCC_PIECE_DEFAULT;
  DevBuf<int2> occ_items;
  DevBuf<int8_t> occ_cls;
  // alego_occ_mark / alego_map_assemble_static: the verdicts in assembly order, the kept count per work item, their scan and the six verdict
  // counts of a call; allocated by the first call and kept
  DevBuf<uint8_t> st_verdict;
  DevBuf<int> st_kept, st_off;
  DevBuf<unsigned long long> st_stats;
  // alego_occ_distance / alego_occ_costmap: the two d2 arrays the passes go between, the envelopes' stacks, the statistics, the cost table and
  // the costs of a call; allocated by the first call and kept
  DevBuf<uint32_t> edt_a, edt_b;
  DevBuf<int2> edt_env;
  DevBuf<unsigned long long> edt_stats;
  DevBuf<uint8_t> edt_table, edt_cost;
};

namespace {
template <class T>
bool A(LmHost* lm, T** p, size_t count, std::string* err) {
  const hipError_t e = lm->mem.get(p, count, true);
  if (e != hipSuccess) { *err = std::string("lm allocation: ") + hipGetErrorString(e); return false; }
  return true;
}

// the nine arrays of the key-frame ring (or of the map store that takes its place, alego_loc_enable): f(array, elements per row)
template <class F> void ring_each(LmCtx& L, F f) {
  f(L.kfs_c, L.kf_cap_c); f(L.kfs_s, L.total_cap); f(L.kfs_n, 2); f(L.kfs_box, 2 * 8); f(L.kf_raw_c, L.kf_cap_c); f(L.kf_raw_s, L.kf_cap_s); f(L.kf_raw_o, L.kf_cap_o);
  f(L.kf_cnt, KF_CNT_W); f(L.kf_pose, KF_POSE_W);
}
bool ring_alloc(LmHost* lm, LmCtx& L, size_t rows, std::string* err) {   // (a pointer that was not allocated is left null)
  bool ok = true;
  ring_each(L, [&](auto*& p, size_t per_row) { p = nullptr; ok = ok && A(lm, &p, rows * per_row, err); });
  return ok;
}
void ring_release(LmHost* lm, LmCtx& L) { ring_each(L, [&](auto*& p, size_t) { lm->mem.release(p); p = nullptr; }); }
// the two sort jobs of one staged key frame (in_c: corner, in_s: surf + outlier): sorted by voxel key of the map's leaf into the row *out_sel names, counted from the
// first row of `slot` (VoxelGrid mode 1).  n_in / n_out: two device words each (corner, surf + outlier); enable, out_sel, overflow: one each.
void kf_sort_job_pair(const LmCtx& L, const alego_params& P, int slot, const float4* in_c, const float4* in_s, const int* n_in, int* n_out, const int* enable, const int* out_sel, int* overflow,
                      std::vector<VoxJob>* out) {
  for (int m = 0; m < 2; ++m) {
    const int cap = m ? L.total_cap : L.kf_cap_c;
    VoxJob j{m ? in_s : in_c, n_in + m, (m ? L.kfs_s : L.kfs_c) + kf_row_at(L, slot, 0) * cap, n_out + m, enable,
             m ? P.lm_leaf_surf : P.lm_leaf_corner, cap, cap, overflow, 0};
    j.mode = 1; j.out_sel = out_sel; j.out_stride = cap;
    j.box_out = L.kfs_box + kf_run_at(L, slot, m, 0) * 8; j.n_sel_out = L.kfs_n + kf_run_at(L, slot, m, 0); j.n_sel_stride = 1;
    out->push_back(j);
  }
}
// ... of a slot's kf_tmp_*, into the row of the slot that LI_KF_PEND_RING names
void kf_sort_jobs(const LmCtx& L, const alego_params& P, int slot, std::vector<VoxJob>* out) {
  int* li = L.li + (size_t)slot * LI_COUNT;
  static_assert(LI_TMPN_S == LI_TMPN_C + 1 && LI_SORT_N1 == LI_SORT_N + 1, "kf_sort_job_pair reads / writes the counts as pairs");
  kf_sort_job_pair(L, P, slot, L.kf_tmp_c + (size_t)slot * L.kf_cap_c, L.kf_tmp_s + (size_t)slot * L.total_cap, li + LI_TMPN_C, li + LI_SORT_N, li + LI_KF_PENDING, li + LI_KF_PEND_RING, li + LI_OVERFLOW, out);
}
}  // namespace

LmHost* lm_host_create(const alego_params& P, const DevCtx& d, int n_slots, int gsize, const std::vector<hipStream_t>& st, std::string* err) {
  LmHost* lm = new LmHost();
  lm->P = P; lm->n_slots = n_slots; lm->gsize = gsize; lm->st = st; lm->frames.assign(n_slots, 0);
  lm->gv.small_max = gv_small_max_env();
  VoxCtx vz; std::memset(&vz, 0, sizeof(VoxCtx));
  lm->vm.assign(st.size(), vz); lm->v2.assign(st.size(), vz); lm->vk.assign(st.size(), vz);
  lm->work.assign(st.size(), MapWork{nullptr, nullptr, 0});
  LmCtx& L = lm->L;
  std::memset(&L, 0, sizeof(L));
  L.K = P.recent_keyframe_num > 0 ? P.recent_keyframe_num : 1;
  L.KR = L.K + 1;
  L.fr_stride = L.KR; L.fr_mod = L.KR;   // every slot's frames live in its own ring
  // the concat + radix-sort path needs the raw maps and 20 B of sort scratch per map point (~42 MB per stream at 16x1800 / K = 50): large
  // batches only carry it when they are configured to use it
  lm->fallback_ok = n_slots <= 64 || !d.opt_map_merge;
  L.in_cap_c = d.fcap[F_LSHARP]; L.in_cap_s = d.N; L.in_cap_o = d.N;
  L.kf_cap_c = d.fcap[F_LSHARP];
  L.kf_cap_s = P.kf_cap_surf > 0 ? std::min(P.kf_cap_surf, d.N) : d.N / 2;
  L.kf_cap_o = P.kf_cap_outlier > 0 ? std::min(P.kf_cap_outlier, d.N) : d.N / 4;
  L.kf_cap_s = std::max(L.kf_cap_s, L.kf_cap_c - L.kf_cap_o);   // (scratch shared by both maps is sized by surf + outlier)
  L.total_cap = L.kf_cap_s + L.kf_cap_o;
  L.map_cap_c = L.K * L.kf_cap_c; L.map_cap_s = L.K * L.total_cap;
  L.gcap = n_slots <= 64 ? (1 << 20) : (1 << 18);
  L.qcap = L.kf_cap_c + L.total_cap;
  {
    const size_t mx = lm_solve_row_bytes_max();
    const char* e = getenv("ALEGO_LM_ROW_LDS");   // development: a smaller budget sends rows through crows (tests: 0 = all of them)
    // more streams per launch than CUs: 72 KB, so that two lm_solve workgroups (254 VGPRs x 4 wavefronts each) share a CU and the few rows beyond the
    // budget come from the L2 (measured at 512 per launch: 446 k -> 452 k scans/s for anything between 56 and 76 KB; at 192 / 128 per launch 96 KB is 1 % better)
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    const size_t dflt = gsize > cus ? (size_t)72 * 1024 : lm_solve_row_bytes_default();
    L.solve_row_bytes = (int)(e ? std::min(mx, (size_t)std::max(0, atoi(e))) : std::min(mx, dflt));
  }
  const size_t B = n_slots;
  bool ok = true;
  ok = ok && A(lm, &L.li, B * LI_COUNT, err) && A(lm, &L.ld, B * LD_COUNT, err);
  ok = ok && A(lm, &L.stage_odom, B * 2 * 8, err);
  ok = ok && A(lm, &L.in_corner, B * L.in_cap_c, err) && A(lm, &L.in_surf, B * L.in_cap_s, err) && A(lm, &L.in_outl, B * L.in_cap_o, err);
  ok = ok && ring_alloc(lm, L, B * L.KR, err);
  ok = ok && A(lm, &L.kf_tmp_c, B * L.kf_cap_c, err) && A(lm, &L.kf_tmp_s, B * L.total_cap, err);
  ok = ok && A(lm, &L.rec, B * L.K, err) && A(lm, &L.rec_prev, B * L.K, err);
  ok = ok && A(lm, &L.U_c, B * L.map_cap_c, err) && A(lm, &L.U_s, B * L.map_cap_s, err) && A(lm, &L.Ucnt_c, B * L.map_cap_c, err) && A(lm, &L.Ucnt_s, B * L.map_cap_s, err);
  ok = ok && A(lm, &L.newkeys, B * 2 * L.total_cap, err) && A(lm, &L.map_bbox, B * 2 * 8, err);
  {
    double* part = nullptr; int* ctl = nullptr; double* state = nullptr;
    ok = ok && A(lm, &part, B * 32, err) && A(lm, &ctl, B * 8, err) && A(lm, &state, B * 64, err);   // LmState is < 64 doubles (checked in kernels_lm.hip)
    L.shard_part = part; L.shard_ctl = ctl; L.shard_state = state;
  }
  ok = ok && A(lm, &L.map_corner_raw, lm->fallback_ok ? B * L.map_cap_c : 1, err) && A(lm, &L.map_surf_raw, lm->fallback_ok ? B * L.map_cap_s : 1, err);
  ok = ok && A(lm, &L.map_corner_ds, B * L.map_cap_c, err) && A(lm, &L.map_surf_ds, B * L.map_cap_s, err);
  ok = ok && A(lm, &L.cur_corner_ds, B * L.kf_cap_c, err) && A(lm, &L.cur_surf_ds, B * L.kf_cap_s, err) && A(lm, &L.cur_outl_ds, B * L.kf_cap_o, err);
  ok = ok && A(lm, &L.cur_total, B * L.total_cap, err) && A(lm, &L.cur_total_ds, B * L.total_cap, err);
  ok = ok && A(lm, &L.grid, B * 2, err) && A(lm, &L.cell_start, B * 2 * ((size_t)L.gcap + 1), err) && A(lm, &L.cell_cur, B * 2 * ((size_t)L.gcap + 1), err);
  ok = ok && A(lm, &L.cell_pts, B * 2 * L.map_cap_s, err);
  ok = ok && A(lm, &L.blocks, B * L.qcap * LMB_W, err) && A(lm, &L.crows, B * L.qcap * LMS_W, err) && A(lm, &L.knn, B * L.qcap * LM_KNN_W, err);   // (lm_rows.h)
  if (!ok) { lm_host_destroy(lm); return nullptr; }
  // identity quaternions (laserMapping.cpp:56-61)
  std::vector<double> ld(B * LD_COUNT, 0.0);
  for (size_t b = 0; b < B; ++b) { ld[b * LD_COUNT + LD_Q_M2O] = 1.0; ld[b * LD_COUNT + LD_Q_O2L] = 1.0; ld[b * LD_COUNT + LD_Q_M2L] = 1.0; }
  DevTry c("lm_host_create", err);
  if (c.up(L.ld, ld)) { lm_host_destroy(lm); return nullptr; }
  std::vector<int> li0(B * LI_COUNT, 0);
  for (size_t b = 0; b < B; ++b) li0[b * LI_COUNT + LI_LATEST] = -1;   // laserMapping.cpp:50
  if (c.up(L.li, li0)) { lm_host_destroy(lm); return nullptr; }
  // VoxelGrid job tables (laserMapping.cpp:37-39,316-319,329-342)
  for (size_t g = 0; g < st.size(); ++g) {
  std::vector<VoxJob> jm, j1, j2, jk;
  for (size_t b = g * gsize; b < B && b < (g + 1) * (size_t)gsize; ++b) {
    int* li = L.li + b * LI_COUNT;
    if (lm->fallback_ok) {   // the maps by concat + radix sort (ALEGO_MAP_MERGE=0)
      jm.push_back(VoxJob{L.map_corner_raw + b * L.map_cap_c, li + LI_KRAW_C, L.map_corner_ds + b * L.map_cap_c, li + LI_KDS_C, li + LI_REBUILD_FB, P.lm_leaf_corner, L.map_cap_c, L.map_cap_c, li + LI_OVERFLOW, 0});
      jm.push_back(VoxJob{L.map_surf_raw + b * L.map_cap_s, li + LI_KRAW_S, L.map_surf_ds + b * L.map_cap_s, li + LI_KDS_S, li + LI_REBUILD_FB, P.lm_leaf_surf, L.map_cap_s, L.map_cap_s, li + LI_OVERFLOW, 0});
    }
    j1.push_back(VoxJob{L.in_corner + b * L.in_cap_c, li + LI_NIN_C, L.cur_corner_ds + b * L.kf_cap_c, li + LI_NCUR_C, li + LI_RUN, P.lm_leaf_corner, L.in_cap_c, L.kf_cap_c, li + LI_OVERFLOW, 0});
    j1.push_back(VoxJob{L.in_surf + b * L.in_cap_s, li + LI_NIN_S, L.cur_surf_ds + b * L.kf_cap_s, li + LI_NCUR_S, li + LI_RUN, P.lm_leaf_surf, L.in_cap_s, L.kf_cap_s, li + LI_OVERFLOW, 0});
    j1.push_back(VoxJob{L.in_outl + b * L.in_cap_o, li + LI_NIN_O, L.cur_outl_ds + b * L.kf_cap_o, li + LI_NCUR_O, li + LI_RUN, P.lm_leaf_outlier, L.in_cap_o, L.kf_cap_o, li + LI_OVERFLOW, 0});
    j1.back().skip_le = LT_OCAP;   // lm_total_merge filters a small /outlier cloud itself (a round with VoxCtx::skip_on)
    j2.push_back(VoxJob{L.cur_total + b * L.total_cap, li + LI_NTOTAL, L.cur_total_ds + b * L.total_cap, li + LI_NTOTAL_DS, li + LI_RUN, P.lm_leaf_surf, L.total_cap, L.total_cap, li + LI_OVERFLOW, 0});
    kf_sort_jobs(L, P, (int)b, &jk);
  }
  const int ns = (int)j1.size() / 3;
  jm.insert(jm.end(), j1.begin(), j1.end());
  jm.insert(jm.end(), jk.begin(), jk.end());
  if (vox_create(&lm->vm[g], jm.data(), (int)jm.size(), err) || vox_create(&lm->v2[g], j2.data(), (int)j2.size(), err) ||
      vox_create(&lm->vk[g], jk.data(), (int)jk.size(), err)) { lm_host_destroy(lm); return nullptr; }
  // Expected work per context: the current-scan clouds and key frames practically never exceed 8192 points (vox_small); a key frame
  // is sorted for ~1 stream in 5 per mapping frame.  Fewer persistent workgroups where little is expected (they loop).
  // (vox_big only has work on the radix path of the maps or for a scan cloud of more than 8192 points)
  // (with 64 rings the scan's own surf clouds exceed 8192 points on every mapping frame: as many workgroups for the large jobs as
  //  mapping frames are expected per round, instead of a handful for the rare one — 64x2048: 1.85 -> see profiles/r02_geo_64x2048*)
  const bool big_scans = d.N > 8 * 8192;
  lm->vm[g].grid_small = 3 * ns + std::max(2, ns / 2);
  // under ALEGO_LM_TOTAL_MERGE the /outlier jobs of small clouds are lm_total_merge's: a third of the scan's jobs less to keep workgroups for (a
  // group whose /outlier clouds exceed LT_OCAP keeps those jobs and loops over them: correct, the workgroups are persistent, and not measured)
  int tm_grid1 = 2 * ns + std::max(2, ns / 2);
  if (const char* e = getenv("ALEGO_VOX_GRID_DIV")) {
    const int dv = std::max(1, atoi(e));
    lm->vm[g].grid_small = std::max(2, lm->vm[g].grid_small / dv); lm->v2[g].grid_small = std::max(1, lm->v2[g].grid_small / dv);
    tm_grid1 = std::max(2, tm_grid1 / dv);
  }
  lm->vm[g].grid_big = (!d.opt_map_merge || big_scans) ? std::max(2, ns / 2) : std::min(8, std::max(2, ns / 2));
  lm->v2[g].grid_big = big_scans ? std::max(2, ns / 2) : std::max(1, ns / 16);
  lm->vk[g].grid_small = 2; lm->vk[g].grid_big = 2;
  lm->tm_grid1.push_back(tm_grid1); lm->tm_par.push_back(0);
  lm->tm_grid.push_back(std::max(1, ns / 16));   // workgroups of the vox_small launch behind lm_total_merge: only the slots it refused have work there
  MapWork& W = lm->work[g];
  W.cap = std::max(4096, 64 * ns);
  if (!A(lm, &W.items, (size_t)W.cap, err) || !A(lm, &W.count, 2, err)) { lm_host_destroy(lm); return nullptr; }
  }
  return lm;
}

void lm_host_destroy(LmHost* lm) {
  if (!lm) return;
  if (lm->comm) { (void)ncclCommDestroy(lm->comm); lm->comm = nullptr; }
  for (auto& v : lm->vm) vox_destroy(&v);
  for (auto& v : lm->v2) vox_destroy(&v);
  for (auto& v : lm->vk) vox_destroy(&v);
  if (lm->vloc_made) vox_destroy(&lm->vloc);
  gv_destroy(&lm->gv);
  lm->mg_pairs.clear(); lm->mg_items.clear(); lm->mg_tail.clear(); lm->mg_moves.clear();
  lm->th_jobs.clear(); lm->th_ints.clear(); lm->th_prot.clear(); lm->th_items.clear(); lm->th_pts.clear(); lm->th_rows.clear(); lm->th_pose.clear();
  lm->mem.clear();
  delete lm;
}

static bool dbg_sync(hipStream_t st, const char* what, std::string* err) {
  static const bool on = getenv("ALEGO_DEBUG_SYNC") != nullptr;
  if (!on) return true;
  hipError_t e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  fprintf(stderr, "[alego dbg] %s: %s\n", what, hipGetErrorString(e));
  if (e != hipSuccess) { *err = std::string(what) + ": " + hipGetErrorString(e); return false; }
  return true;
}

// the local maps of the slots whose window changed (LI_REBUILD, set by lm_prepare) + the VoxelGrid filters of the scan's three
// clouds + the sort of a pending key frame, then the k-NN grids
static int map_sequence(LmHost* lm, const DevCtx& d, const LmCtx& L, int g, hipStream_t st, std::string* err) {
  if (!d.opt_map_merge) {
    if (!lm->fallback_ok) { *err = "ALEGO_MAP_MERGE=0 needs the handle to be created with it (more than 64 slots)"; return ALEGO_ERR_ARG; }
    launch_lm_concat(d, L, st);
    if (!dbg_sync(st, "lm_concat", err)) return ALEGO_ERR_HIP;
  }
  VoxCtx V1 = lm->vm[g];
  if (d.opt_lm_total_merge) { V1.skip_on = 1; V1.grid_small = lm->tm_grid1[g]; }   // (the /outlier jobs of small clouds are lm_total_merge's)
  if (int r = vox_run(V1, st, err)) return r;
  if (!dbg_sync(st, "vox round 1", err)) return ALEGO_ERR_HIP;
  launch_map_update(d, L, lm->work[g], st);   // (also closes the key-frame sort's bookkeeping when the maps come from the radix path)
  if (!dbg_sync(st, "map_update", err)) return ALEGO_ERR_HIP;
  if (d.opt_map_merge) {
    launch_map_accum(d, L, lm->work[g], st);
    if (!dbg_sync(st, "map_accum", err)) return ALEGO_ERR_HIP;
  }
  launch_lm_grid(d, L, st);
  if (!dbg_sync(st, "lm_grid", err)) return ALEGO_ERR_HIP;
  return 0;
}

// sum of the partial normal equations over the ranks, in place, on the registration's stream (RCCL over xGMI)
static int lm_allreduce(void* ctx, double* buf, size_t count, hipStream_t st) {
  LmHost* lm = static_cast<LmHost*>(ctx);
  const ncclResult_t r = ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, lm->comm, st);
  if (r != ncclSuccess) { lm->dist_err = std::string("ncclAllReduce: ") + ncclGetErrorString(r); return ALEGO_ERR_HIP; }
  return 0;
}

// odom_valid[s - slot0]: whether slot s has an /odom/lidar message for this scan (false on its first scan)
// A (optional): LaserMapping of this scan runs on A->back, behind the hand-over kernel lm_stage on the front end's stream.
struct LmAsync { hipStream_t front, back; hipEvent_t staged, back_same, back_other; long k; };   // k: scans handed over before this one (its parity picks the staging buffer)
static int lm_sequence(LmHost* lm, const DevCtx& d, int stage, const std::vector<char>& odom_valid, std::string* err, hipStream_t st_override = nullptr, const LmAsync* A = nullptr) {
  // the slots of one launch view always belong to one stream group
  const int g = d.slot0 / lm->gsize;
  hipStream_t st = A ? A->back : (st_override ? st_override : lm->st[g]);
  LmCtx L = lm->L;
  L.vox_bbox = lm->vm[g].bbox; L.vox_slot0 = g * lm->gsize;
  int n_run = 0, n_norun = 0;
  for (int i = 0; i < d.n_launch; ++i) {
    long& f = lm->frames[d.slot0 + i];
    const bool run = odom_valid[i] && (f % lm->P.lm_every) == 0;
    if (odom_valid[i]) ++f;
    run ? ++n_run : ++n_norun;
  }
  const int hint = n_run == 0 ? 0 : (n_norun == 0 ? 1 : -1);  // -1: slots out of phase, no launch skipping
  int par = 0;
  if (A) {
    par = (int)(A->k & 1);
    // stage_odom[par] was last read by the LaserMapping of scan k - 2; the cloud inputs by the last mapping frame (k - 1 at the latest)
    if (A->k >= 2 && hipStreamWaitEvent(A->front, A->back_same, 0) != hipSuccess) { *err = "hipStreamWaitEvent failed"; return ALEGO_ERR_HIP; }
    if (hint != 0 && A->k >= 1 && hipStreamWaitEvent(A->front, A->back_other, 0) != hipSuccess) { *err = "hipStreamWaitEvent failed"; return ALEGO_ERR_HIP; }
    launch_lm_stage(d, L, hint, par, A->front);
    if (hipEventRecord(A->staged, A->front) != hipSuccess || hipStreamWaitEvent(st, A->staged, 0) != hipSuccess) { *err = "event hand-over to the LaserMapping stream failed"; return ALEGO_ERR_HIP; }
    stage = 2;
  }
  launch_lm_prepare(d, L, stage, hint, par, st);
  if (!dbg_sync(st, "lm_prepare", err)) return ALEGO_ERR_HIP;
  if (n_run == 0) return 0;
  if (L.loc_on) {   // the window of every slot that maps this scan, from the pose lm_prepare has just associated
    launch_loc_select(d, L, st);
    if (!dbg_sync(st, "loc_select", err)) return ALEGO_ERR_HIP;
  }
  if (int r = map_sequence(lm, d, L, g, st, err)) return r;   // (includes the VoxelGrid filters of the scan's three clouds)
  if (d.opt_lm_total_merge) {
    // laser_outlier_ds_ of a small /outlier cloud and laser_surf_total_ds_ by one light workgroup per slot; the slots it refuses are on the
    // round-2 context's work lists behind it, for a vox_small launch of a few persistent workgroups (lm_total_merge_grid)
    VoxCtx V2 = lm->v2[g];
    int* const cnt = V2.cnt;
    const int par = lm->tm_par[g];
    lm->tm_par[g] ^= 1;
    // this launch's list sizes: one of two sets that only lm_total_merge writes (vox_plan's own pair is cnt[0..1], so rounds with the option off
    // in between leave them alone), zeroed by the lm_total_merge launch before it, which used the other set
    V2.cnt = cnt + 2 + 2 * par;
    launch_lm_total_merge(d, L, LtLists{V2.list_small, V2.list_big, V2.cnt, cnt + 2 + 2 * (par ^ 1), VX_SMALL_MAX}, st);
    if (!dbg_sync(st, "lm_total_merge", err)) return ALEGO_ERR_HIP;
    V2.grid_small = V2.grid_big = lm->tm_grid[g];
    if (int r = vox_run_listed(V2, st, err)) return r;
  } else {
    launch_lm_total(d, L, st);
    if (int r = vox_run(lm->v2[g], st, err)) return r;
  }
  if (!dbg_sync(st, "vox total", err)) return ALEGO_ERR_HIP;
  if (int r = launch_lm_register(d, L, st, lm->comm ? &lm_allreduce : nullptr, lm)) { *err = "sharded registration: " + lm->dist_err; return r; }
  if (!dbg_sync(st, "lm_register", err)) return ALEGO_ERR_HIP;
  return 0;
}

// NOTE: the VoxelGrid rounds always cover every slot of the stream group; slots outside the launch view
// have LI_RUN == 0 from their own last prepare only if they were prepared in this call, so the
// single-slot entry points clear the run flags of the other slots of the group first.
static void clear_run_flags_outside(LmHost* lm, const DevCtx& d) {
  const int g = d.slot0 / lm->gsize;
  const int lo = g * lm->gsize, hi = std::min(lm->n_slots, lo + lm->gsize);
  if (d.slot0 == lo && d.slot0 + d.n_launch == hi) return;
  for (int s = lo; s < hi; ++s) {
    if (s >= d.slot0 && s < d.slot0 + d.n_launch) continue;
    (void)hipMemsetAsync(lm->L.li + (size_t)s * LI_COUNT + LI_RUN, 0, sizeof(int), lm->st[g]);  // LI_REBUILD is always 0 between map sequences
  }
}

int lm_host_enqueue(LmHost* lm, const DevCtx& d, const std::vector<char>& odom_valid, std::string* err, hipStream_t st_override) {
  if (!st_override) clear_run_flags_outside(lm, d);   // (alego_stream_run: the other slots of the group are look-ahead lanes, LaserMapping never ran on them)
  return lm_sequence(lm, d, 1, odom_valid, err, st_override);
}
// The batch path: the view covers a whole stream group; LaserMapping of the scan goes to `back`, lm_stage to `front`.
int lm_host_enqueue_async(LmHost* lm, const DevCtx& d, const std::vector<char>& odom_valid, std::string* err, hipStream_t front, hipStream_t back,
                          hipEvent_t staged, hipEvent_t back_same, hipEvent_t back_other, long k) {
  const LmAsync A{front, back, staged, back_same, back_other, k};
  return lm_sequence(lm, d, 1, odom_valid, err, nullptr, &A);
}

int lm_host_process_host(LmHost* lm, const DevCtx& dfull, const alego_point* corner_last, int n_corner, const alego_point* surf_last,
                         int n_surf, const alego_point* outlier, int n_outlier, const alego_pose* odom, alego_pose* map_pose,
                         std::string* err) {
  const LmCtx& L = lm->L;
  if (n_corner > L.in_cap_c || n_surf > L.in_cap_s || n_outlier > L.in_cap_o) { *err = "alego_lm_process: input cloud exceeds capacity"; return ALEGO_ERR_CAPACITY; }
  DevCtx d = dfull;
  d.slot0 = 0; d.n_launch = 1;
  hipStream_t st = lm->st[0];
  if ((n_corner > 0 && !corner_last) || (n_surf > 0 && !surf_last) || (n_outlier > 0 && !outlier) || n_corner < 0 || n_surf < 0 || n_outlier < 0) { *err = "alego_lm_process: null cloud / negative count"; return ALEGO_ERR_ARG; }
  DevTry c("alego_lm_process", err, "upload");
  c.up(L.in_corner, corner_last, (size_t)n_corner, st).up(L.in_surf, surf_last, (size_t)n_surf, st).up(L.in_outl, outlier, (size_t)n_outlier, st);
  const int nin[3] = {n_corner, n_surf, n_outlier};
  c.up(L.li + LI_NIN_C, nin, st);
  double po[7] = {odom->t[0], odom->t[1], odom->t[2], odom->q[0], odom->q[1], odom->q[2], odom->q[3]};
  c.up(poses_of(d, 0) + PO_ODOM_T, po, st);   // (the single-scan entry points work on slot 0)
  const int one = 1;
  if (c.up(scal_of(d, 0) + SC_ODOM_VALID, &one, 1, st).wait(st)) return c;
  clear_run_flags_outside(lm, d);
  if (int r = lm_sequence(lm, d, 0, std::vector<char>(1, 1), err)) return r;
  double out[PO_W], ld[LD_COUNT];
  int li[LI_COUNT];
  if (c.at("kernels").down(out, poses_of(d, 0), st).down(ld, L.ld, st).down(li, L.li, st).wait(st)) return c;
  if (li[LI_OVERFLOW]) {   // reported by the call that caused it, then cleared
    const int zero = 0;
    (void)dev_up(L.li + LI_OVERFLOW, &zero, 1);
    *err = li[LI_OVERFLOW] == 2 ? "alego_lm_process: launch logic out of sync"
         : li[LI_OVERFLOW] == 8 ? "alego_lm_process: the key-frame window has a point outside the voxel-key range of -2^20 .. 2^20 - 1 leaves per axis (no local map was built)"
                                : "alego_lm_process: device capacity exceeded (cloud truncated)";
    return ALEGO_ERR_CAPACITY;
  }
  if (map_pose) {
    for (int i = 0; i < 3; ++i) map_pose->t[i] = out[PO_MAP_T + i];
    for (int i = 0; i < 4; ++i) map_pose->q[i] = out[PO_MAP_Q + i];
    for (int i = 0; i < 6; ++i) map_pose->params[i] = ld[LD_PARAMS + i];
    map_pose->valid = 1;
  }
  return li[LI_FLAGS];
}

const double* lm_host_stage_odom(LmHost* lm) { return lm->L.stage_odom; }
void lm_host_get_params(LmHost* lm, int slot, double* p6) {
  (void)dev_down(p6, lm->L.ld + (size_t)slot * LD_COUNT + LD_PARAMS, 6);
}
int lm_host_set_params(LmHost* lm, int slot, const double* p6, std::string* err) {
  return DevTry("set_lm_params", err).up(lm->L.ld + (size_t)slot * LD_COUNT + LD_PARAMS, p6, 6);
}
// LI_OVERFLOW stays set until it has been reported to the host once (the batch path only looks at the end of a run)
int lm_host_get_flags(LmHost* lm, int slot) {
  int li[LI_COUNT];
  if (dev_down(li, lm->L.li + (size_t)slot * LI_COUNT) != hipSuccess) return ALEGO_ERR_HIP;
  if (li[LI_OVERFLOW]) {
    const int zero = 0;
    (void)dev_up(lm->L.li + (size_t)slot * LI_COUNT + LI_OVERFLOW, &zero, 1);
    return ALEGO_ERR_CAPACITY;
  }
  return li[LI_FLAGS];
}
void lm_host_get_counts(LmHost* lm, int slot, int* o) {  // o[7]
  int li[LI_COUNT];
  (void)dev_down(li, lm->L.li + (size_t)slot * LI_COUNT);
  o[0] = li[LI_KRAW_C]; o[1] = li[LI_KRAW_S]; o[2] = li[LI_KDS_C]; o[3] = li[LI_KDS_S]; o[4] = li[LI_NCUR_C]; o[5] = li[LI_NTOTAL_DS]; o[6] = li[LI_NREBUILD];
}

// ---- key-frame pass-through (alego_lm_get_keyframe / set_keypose / reset_window / apply_correction / add_keyframe) ----
static hipStream_t stream_of_slot(LmHost* lm, int slot) { return lm->st[slot / lm->gsize]; }
int lm_host_keyframe_count(LmHost* lm, int slot) {
  int n = 0;
  if (dev_wait(stream_of_slot(lm, slot)) != hipSuccess || dev_down(&n, lm->L.li + (size_t)slot * LI_COUNT + LI_NKF, 1) != hipSuccess) return ALEGO_ERR_HIP;
  return n;
}
// One frame to the host: id, pose and counts always, each cloud the caller gave a buffer for (ALEGO_ERR_CAPACITY when one is too small); n / src: points and device cloud per kind
static int frame_to_host(const char* what, int id, const float* pose_dev, const int* n, const float4* const* src, alego_keyframe* out, std::string* err) {
  float kp[KF_POSE_W];
  DevTry c(what, err, "copy");
  if (c.down(kp, pose_dev)) return c;
  out->id = id;
  for (int k = 0; k < 6; ++k) out->pose[k] = kp[k];
  out->n_corner = n[KF_CORNER]; out->n_surf = n[KF_SURF]; out->n_outlier = n[KF_OUTL];
  alego_point* const dst[KF_KINDS] = {out->corner, out->surf, out->outlier};   // (KF_CORNER, KF_SURF, KF_OUTL)
  const int cap[KF_KINDS] = {out->corner_cap, out->surf_cap, out->outlier_cap};
  for (int k = 0; k < KF_KINDS; ++k) if (dst[k] && n[k] > cap[k]) { *err = std::string(what) + ": buffer too small"; return ALEGO_ERR_CAPACITY; }
  for (int k = 0; k < KF_KINDS; ++k) if (dst[k]) c.down(dst[k], src[k], (size_t)n[k]);
  return c;
}
int lm_host_get_keyframe(LmHost* lm, int slot, int kf_id, alego_keyframe* out, std::string* err) {
  const LmCtx& L = lm->L;
  const int nkf = lm_host_keyframe_count(lm, slot);
  if (nkf < 0) { *err = "get_keyframe: device error"; return nkf; }
  if (kf_id < 0) kf_id = nkf - 1;
  if (kf_id < 0 || kf_id >= nkf || kf_id < nkf - L.K) { *err = "get_keyframe: key frame not resident (only the recent_keyframe_num newest are)"; return ALEGO_ERR_ARG; }
  const KfRingRow R = kf_ring_row_at(L, slot, kf_entry(L, kf_id), KF_CORNER);
  int cnt[KF_CNT_W];
  if (int r = DevTry("get_keyframe", err, "copy").down(cnt, R.cnt)) return r;
  const float4* const src[KF_KINDS] = {R.raw, kf_raw_of(L, R.row, KF_SURF), kf_raw_of(L, R.row, KF_OUTL)};
  return frame_to_host("get_keyframe", kf_id, R.pose, cnt, src, out, err);
}
// a frame of the host into ring row R: key pose, counts, the three clouds
static void frame_to_row(const LmCtx& L, const KfRingRow& R, const alego_kf_in& f, DevTry* c) {
  const float kp[KF_POSE_W] = {f.pose[0], f.pose[1], f.pose[2], f.pose[3], f.pose[4], f.pose[5], 0.f, 0.f};
  const int cnt[KF_CNT_W] = {f.n_corner, f.n_surf, f.n_outlier, 0};   // (KF_CORNER, KF_SURF, KF_OUTL)
  const alego_point* const src[KF_KINDS] = {f.corner, f.surf, f.outlier};
  c->up(R.pose, kp).up(R.cnt, cnt);
  for (int k = 0; k < KF_KINDS; ++k) c->up(kf_raw_of(L, R.row, k), src[k], (size_t)cnt[k]);
}
static int retransform(LmHost* lm, const DevCtx& dfull, int slot, int ring, std::string* err) {
  DevCtx d = dfull;
  d.slot0 = slot; d.n_launch = 1;
  hipStream_t st = stream_of_slot(lm, slot);
  const int g = slot / lm->gsize;
  const int zero = 0;
  int* li = lm->L.li + (size_t)slot * LI_COUNT;
  // a key frame saved by the last mapping frame may still wait in kf_tmp_* for its sort: flush it before the buffer is reused
  if (int r = vox_run(lm->vk[g], st, err)) return r;
  (void)dev_up(li + LI_KF_PENDING, &zero, 1, st);
  launch_lm_retransform(d, lm->L, ring, st);
  // the row's clouds were (re)written outside the regular sequence: sort it into the ring now, and the next map update rebuilds its voxel lists
  std::string e;
  (void)vox_run(lm->vk[g], st, &e);
  (void)dev_up(li + LI_KF_PENDING, &zero, 1, st);
  (void)dev_up(li + LI_UVALID, &zero, 1, st);
  return DevTry("retransform", err, "key-frame transform").wait(st);
}
int lm_host_set_keypose(LmHost* lm, const DevCtx& dfull, int slot, int kf_id, const float* pose6, std::string* err) {
  const LmCtx& L = lm->L;
  const int nkf = lm_host_keyframe_count(lm, slot);
  if (nkf < 0) return nkf;
  if (kf_id < 0 || kf_id >= nkf || kf_id < nkf - L.K) { *err = "set_keypose: key frame not resident"; return ALEGO_ERR_ARG; }
  DevTry c("set_keypose", err, "copy");
  if (c.up(kf_pose_of(L, kf_row(L, slot, kf_id)), pose6, 6)) return c;
  if (L.arc_frames_cap > 0) {   // the archived copy of the frame (alego_map_enable) follows
    int stat[AS_W];
    if (c.down(stat, arc_stat_of(L, slot))) return c;
    if (kf_id < stat[AS_FRAMES] && c.up(arc_pose_of(L, slot, kf_id), pose6, 6)) return c;
  }
  return retransform(lm, dfull, slot, kf_entry(L, kf_id), err);
}
int lm_host_reset_window(LmHost* lm, int slot, std::string* err) {
  int* li = lm->L.li + (size_t)slot * LI_COUNT;
  DevTry c("reset_window", err);
  c.wait(stream_of_slot(lm, slot));
  kf_reset_window([&](int w, int v) { c.up(li + w, &v, 1); });
  return c;
}
int lm_host_apply_correction(LmHost* lm, const DevCtx& dfull, int slot, const double* rc12, std::string* err) {
  DevPool tmp;
  double* dev = nullptr;
  hipStream_t st = stream_of_slot(lm, slot);
  if (tmp.get(&dev, 12, false) != hipSuccess) { *err = "apply_correction: allocation failed"; return ALEGO_ERR_HIP; }
  DevTry c("apply_correction", err);
  if (c.up(dev, rc12, 12)) return c;
  launch_lm_apply_correction(dfull, lm->L, slot, dev, st);
  return c.wait(st);
}
int lm_host_add_keyframe(LmHost* lm, const DevCtx& dfull, int slot, const float* pose6, const alego_point* corner, int nc, const alego_point* surf, int ns,
                         const alego_point* outlier, int no, std::string* err) {
  const LmCtx& L = lm->L;
  const alego_kf_in f{{pose6[0], pose6[1], pose6[2], pose6[3], pose6[4], pose6[5]}, corner, nc, surf, ns, outlier, no};
  if (!kf_in_valid(f)) { *err = "add_keyframe: null cloud / negative count"; return ALEGO_ERR_ARG; }
  if (nc > L.kf_cap_c || ns > L.kf_cap_s || no > L.kf_cap_o) { *err = "add_keyframe: cloud exceeds the key-frame capacity"; return ALEGO_ERR_CAPACITY; }
  const int nkf = lm_host_keyframe_count(lm, slot);
  if (nkf < 0) return nkf;
  int* li = L.li + (size_t)slot * LI_COUNT;
  DevTry c("add_keyframe", err);
  {
    // A full window advances by ONE frame per mapping frame (pop the oldest, push the newest, laserMapping.cpp:224-237): it keeps its
    // K - 1 other frames however many frames were added in between, and falls behind the newest frames by one for every extra frame.
    // The device holds the K + 1 newest frames, so the window may lag by one: the frame inserted here (id nkf) is refused when the
    // oldest frame the next window still needs, rec[1], would no longer be among the K + 1 newest, i.e. rec[1] < nkf - K.
    int rec_cnt = 0;
    if (c.down(&rec_cnt, li + LI_REC_CNT, 1)) return c;
    if (rec_cnt >= L.K && L.K >= 2) {
      int rec1 = 0;
      if (c.down(&rec1, L.rec + (size_t)slot * L.K + 1, 1)) return c;
      if (rec1 < nkf - L.K) {
        *err = "add_keyframe: the full local-map window already lags one frame behind the newest key frames (it advances by one frame per mapping frame); "
               "insert at most one extra key frame per window length, or call alego_lm_reset_window first (the window is then rebuilt from the newest frames)";
        return ALEGO_ERR_CAPACITY;
      }
    }
  }
  const int nkf1 = nkf + 1, one = 1;
  frame_to_row(L, kf_ring_row_at(L, slot, kf_entry(L, nkf), KF_CORNER), f, &c);
  if (c.up(li + LI_NKF, &nkf1, 1).up(li + LI_DIRTY, &one, 1)) return c;
  if (int r = retransform(lm, dfull, slot, kf_entry(L, nkf), err)) return r;
  if (L.arc_frames_cap > 0) {   // the archive (alego_map_enable) takes the inserted frame like a saved one
    DevCtx d = dfull;
    d.slot0 = slot; d.n_launch = 1;
    launch_map_archive(d, L, 1, stream_of_slot(lm, slot));
    c.at("archive append").wait(stream_of_slot(lm, slot));
  }
  return c;
}

// ---- one registration sharded over the ranks of a communicator (alego_dist_*) ----
int lm_host_dist_unique_id(char* id128) {
  static_assert(sizeof(ncclUniqueId) <= 128, "ALEGO_DIST_ID_BYTES");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return ALEGO_ERR_HIP;
  std::memset(id128, 0, 128);
  std::memcpy(id128, &u, sizeof(u));
  return 0;
}
int lm_host_dist_init(LmHost* lm, int rank, int world, const char* id128, std::string* err) {
  if (lm->comm) { *err = "alego_dist_init: already initialised"; return ALEGO_ERR_ARG; }
  if (lm->rc_on) { *err = "alego_dist_init: not available with alego_regcov_enable (the sharded solver never holds a registration's normal equations in one place)"; return ALEGO_ERR_ARG; }
  if (lm->rm_on) { *err = "alego_dist_init: not available with alego_remap_enable (the sharded solver's step is taken apart from its evaluations)"; return ALEGO_ERR_ARG; }
  if (world < 1 || rank < 0 || rank >= world) { *err = "alego_dist_init: rank / world out of range"; return ALEGO_ERR_ARG; }
  if (lm->st.size() != 1) { *err = "alego_dist_init: a sharded registration needs a handle with one stream group (collectives of one communicator must not overlap)"; return ALEGO_ERR_ARG; }
  ncclUniqueId u;
  std::memcpy(&u, id128, sizeof(u));
  const ncclResult_t r = ncclCommInitRank(&lm->comm, world, u, rank);
  if (r != ncclSuccess) { lm->comm = nullptr; *err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); return ALEGO_ERR_HIP; }
  lm->L.shard_rank = rank; lm->L.shard_world = world;
  return 0;
}
// the collective of one solver evaluation on its own: `iters` in-place ncclAllReduce(sum, 32 doubles) back to back on the registration's
// stream between two events (every rank has to call it: it IS a collective); microseconds per all-reduce, enqueue + completion included
int lm_host_dist_probe(LmHost* lm, int iters, double* usec, std::string* err) {
  if (!lm->comm) { *err = "alego_dist_allreduce_probe: no communicator (alego_dist_init first)"; return ALEGO_ERR_ARG; }
  if (iters < 1 || !usec) { *err = "alego_dist_allreduce_probe: iters / output"; return ALEGO_ERR_ARG; }
  hipStream_t st = lm->st[0];
  DevPool tmp;
  double* buf = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (tmp.get(&buf, 32, false) != hipSuccess || hipMemsetAsync(buf, 0, 32 * sizeof(double), st) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { *err = "alego_dist_allreduce_probe: allocation failed"; return ALEGO_ERR_HIP; }
  int rc = 0;
  for (int i = 0; i < 8 && !rc; ++i) rc = lm_allreduce(lm, buf, 32, st);   // warm the channels
  (void)hipEventRecord(e0, st);
  for (int i = 0; i < iters && !rc; ++i) rc = lm_allreduce(lm, buf, 32, st);
  (void)hipEventRecord(e1, st);
  const hipError_t se = dev_wait(st);
  float ms = 0.f;
  if (!rc && se == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); tmp.clear();
  if (rc) { *err = lm->dist_err; return rc; }
  if (int r = DevTry("alego_dist_allreduce_probe", err).took(se, "a stream")) return r;
  *usec = 1e3 * (double)ms / iters;
  return 0;
}
int lm_host_dist_shutdown(LmHost* lm) {
  if (!lm->comm) return 0;
  (void)dev_wait(lm->st);
  (void)ncclCommDestroy(lm->comm);
  lm->comm = nullptr; lm->L.shard_rank = 0; lm->L.shard_world = 0;
  return 0;
}

// tests: only the query slice of rank `rank` of `world` is associated (no communicator: the fused solver then works on that slice alone)
int lm_host_debug_slice(LmHost* lm, int rank, int world, std::string* err) {
  if (lm->comm) { *err = "ALEGO_SHARD_SLICE: a communicator is active"; return ALEGO_ERR_ARG; }
  if (world < 0 || (world > 0 && (rank < 0 || rank >= world))) { *err = "ALEGO_SHARD_SLICE: rank / world out of range"; return ALEGO_ERR_ARG; }
  lm->L.shard_rank = rank; lm->L.shard_world = world;
  return 0;
}

// ALEGO_MAP_MERGE switched at run time (tests): the voxel lists no longer describe what the other path did in between
int lm_host_set_map_merge(LmHost* lm, int on, std::string* err) {
  if (!on && !lm->fallback_ok) { *err = "ALEGO_MAP_MERGE=0 needs the handle to be created with it (more than 64 slots)"; return ALEGO_ERR_ARG; }
  if (!on && lm->L.loc_on) { *err = "ALEGO_MAP_MERGE=0: a localising handle builds its local maps from the map store's sorted runs only"; return ALEGO_ERR_ARG; }
  (void)dev_wait(lm->st);
  const int zero = 0;
  DevTry c("set_map_merge", err, "copy");
  for (int b = 0; b < lm->n_slots; ++b) c.up(lm->L.li + (size_t)b * LI_COUNT + LI_UVALID, &zero, 1);
  return c;
}

int lm_host_debug_get(LmHost* lm, int slot, const char* name, void* out, int cap_bytes, int* count, int* dtype, std::string* err) {
  const LmCtx& L = lm->L;
  int li[LI_COUNT];
  (void)dev_down(li, L.li + (size_t)slot * LI_COUNT);
  const std::string s(name);
  const void* src = nullptr;
  size_t n = 0;
  int dt = 0, esz = 4;
  auto set = [&](const void* p, size_t cnt, int t) { src = p; n = cnt; dt = t; esz = t == 1 ? 8 : t == 3 ? 1 : 4; };
  const size_t b = slot;
  if (s == "lm_info") set(L.li + b * LI_COUNT, LI_COUNT, 2);
  else if (s == "lm_state") set(L.ld + b * LD_COUNT, LD_COUNT, 1);
  else if (s == "lm_corner_map") set(L.map_corner_raw + b * L.map_cap_c, (size_t)li[LI_KRAW_C] * 4, 0);
  else if (s == "lm_surf_map") set(L.map_surf_raw + b * L.map_cap_s, (size_t)li[LI_KRAW_S] * 4, 0);
  else if (s == "lm_corner_map_ds") set(L.map_corner_ds + b * L.map_cap_c, (size_t)li[LI_KDS_C] * 4, 0);
  else if (s == "lm_surf_map_ds") set(L.map_surf_ds + b * L.map_cap_s, (size_t)li[LI_KDS_S] * 4, 0);
  else if (s == "lm_corner_ds") set(L.cur_corner_ds + b * L.kf_cap_c, (size_t)li[LI_NCUR_C] * 4, 0);
  else if (s == "lm_surf_ds") set(L.cur_surf_ds + b * L.kf_cap_s, (size_t)li[LI_NCUR_S] * 4, 0);
  else if (s == "lm_outlier_ds") set(L.cur_outl_ds + b * L.kf_cap_o, (size_t)li[LI_NCUR_O] * 4, 0);
  else if (s == "lm_surf_total_ds") set(L.cur_total_ds + b * L.total_cap, (size_t)li[LI_NTOTAL_DS] * 4, 0);
  else if (s == "lm_blocks") set(L.blocks + b * L.qcap * LMB_W, (size_t)L.qcap * LMB_W, 1);   // rows as lm_row_of gives them (lm_rows.h): corner queries from 0, surf queries from kf_cap_c
  else if (s == "lm_knn") set(L.knn + b * L.qcap * LM_KNN_W, (size_t)L.qcap * LM_KNN_W, 2);   // the same rows; -1 x LM_KNN_W = rejected
  else if (s == "lm_keyposes") set(kf_pose_of(L, kf_row_at(L, slot, 0)), (size_t)(L.loc_on ? L.loc_n : L.fr_mod) * KF_POSE_W, 0);   // (localisation: the map store's)
  else if (s == "lm_window") set(L.rec + b * L.K, (size_t)li[LI_REC_CNT], 2);   // frame ids of recent_*_keyframes_
  else if (s == "lm_kf_corner_map" || s == "lm_kf_surf_map") {   // newest key frame in the map frame, sorted by voxel key (surf = surf + outlier)
    const int nkf = li[LI_NKF];
    if (nkf <= 0) { *count = 0; *dtype = 0; return 0; }
    const int m = s == "lm_kf_corner_map" ? 0 : 1;
    int n = 0;
    (void)dev_down(&n, L.kfs_n + kf_run_at(L, slot, m, kf_entry(L, nkf - 1)), 1);
    if (m == 0) set(L.kfs_c + kf_row(L, slot, nkf - 1) * L.kf_cap_c, (size_t)n * 4, 0);
    else set(L.kfs_s + kf_row(L, slot, nkf - 1) * L.total_cap, (size_t)n * 4, 0);
  }
  else if (s == "lm_voxel_keys_c" || s == "lm_voxel_keys_s") {   // the sorted voxel-key list of a map as pairs of i32 (lo, hi)
    const int m = s == "lm_voxel_keys_c" ? 0 : 1;
    set(m == 0 ? (const void*)(L.U_c + b * L.map_cap_c) : (const void*)(L.U_s + b * L.map_cap_s), (size_t)li[LI_NU_C + m] * 2, 2);
  }
  else if (s.rfind("ls_", 0) == 0 && s.find(':') != std::string::npos) {   // "ls_<what>:<f>": row f of a localising handle's map store (the slot argument plays no part)
    const std::string w = s.substr(0, s.find(':'));
    const int f = atoi(s.c_str() + s.find(':') + 1);
    if (!L.loc_on || f < 0 || f >= L.loc_n) { *err = std::string("debug_get: ") + name + ": no such frame in a map store"; return ALEGO_ERR_ARG; }
    int cnt[KF_CNT_W], run[2];
    for (int m = 0; m < 2; ++m) (void)dev_down(run + m, L.kfs_n + kf_run_at(L, 0, m, f), 1);
    (void)dev_down(cnt, kf_cnt_of(L, kf_row_at(L, 0, f)));
    const KfClouds C = kf_clouds_row_at(L, 0, f, cnt);
    if (w == "ls_corner") set(L.kfs_c + kf_row_at(L, 0, f) * L.kf_cap_c, (size_t)std::min(std::max(run[0], 0), L.kf_cap_c) * 4, 0);
    else if (w == "ls_surf") set(L.kfs_s + kf_row_at(L, 0, f) * L.total_cap, (size_t)std::min(std::max(run[1], 0), L.total_cap) * 4, 0);
    else if (w == "ls_box_c" || w == "ls_box_s") set(L.kfs_box + kf_run_at(L, 0, w == "ls_box_s", f) * 8, 8, 0);
    else if (w == "ls_raw_c" || w == "ls_raw_s" || w == "ls_raw_o") { const int k = w == "ls_raw_c" ? KF_CORNER : (w == "ls_raw_s" ? KF_SURF : KF_OUTL); set(C.pts[k], (size_t)std::max(C.n[k], 0) * 4, 0); }
    else if (w == "ls_pose") set(kf_pose_of(L, kf_row_at(L, 0, f)), KF_POSE_W, 0);
    else if (w == "ls_counts") {   // the two run counts, then the stored points per kind
      const int o[2 + KF_KINDS] = {run[0], run[1], cnt[KF_CORNER], cnt[KF_SURF], cnt[KF_OUTL]};
      if ((size_t)cap_bytes < sizeof(o)) { *err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
      std::memcpy(out, o, sizeof(o));
      *count = 2 + KF_KINDS; *dtype = 2;
      return 0;
    }
    else { *err = std::string("debug_get: unknown name ") + name; return ALEGO_ERR_ARG; }
  }
  else { *err = std::string("debug_get: unknown name ") + name; return ALEGO_ERR_ARG; }
  if ((size_t)cap_bytes < n * esz) { *err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
  if (int r = DevTry("debug_get", err).took(dev_down_bytes(out, src, n * esz), "copy")) return r;
  *count = (int)n; *dtype = dt;
  return 0;
}

// 0 while no slot has saved a key frame (scans too: or run a mapping frame), else ALEGO_ERR_ARG: what is enabled on a handle has to exist before the first one
static int rings_empty(LmHost* lm, const char* what, bool scans_too, std::string* err) {
  std::vector<int> li((size_t)lm->n_slots * LI_COUNT);
  if (int r = DevTry(what, err).down(li, lm->L.li)) return r;
  for (int s = 0; s < lm->n_slots; ++s)
    if (li[(size_t)s * LI_COUNT + LI_NKF] != 0 || (scans_too && li[(size_t)s * LI_COUNT + LI_FRAME] != 0)) {
      *err = std::string(what) + (scans_too ? ": call it before the first scan / key frame of any slot" : ": call it before the first key frame is saved");
      return ALEGO_ERR_ARG;
    }
  return 0;
}

// ---- the global map (alego_map_* / alego_lm_get_local_map / alego_voxel_grid) ----
// (once per handle: the API owns that flag and refuses a second call, as it does for lm_host_graph_enable)
int lm_host_map_enable(LmHost* lm, int max_frames, int max_points, std::string* err) {
  LmCtx& L = lm->L;
  if (max_frames <= 0 || max_points <= 0) { *err = "map_enable: capacities must be positive"; return ALEGO_ERR_ARG; }
  if (int r = rings_empty(lm, "map_enable", false, err)) return r;   // the archive holds frame ids 0, 1, ...: it has to exist before the first key frame
  const size_t B = lm->n_slots;
  LmCtx T = L;
  bool ok = A(lm, &T.arc_pts, B * max_points, err) && A(lm, &T.arc_tab, B * max_frames * AT_W, err) && A(lm, &T.arc_pose, B * max_frames * KF_POSE_W, err) &&
            A(lm, &T.arc_stat, B * AS_W, err) && A(lm, &T.arc_stamp, B * max_frames, err) && A(lm, &T.arc_stamped, B, err) &&
            A(lm, &lm->arc_off, (size_t)max_frames + 1, err);
  if (!ok) return ALEGO_ERR_HIP;
  if (int r = gv_reserve(&lm->gv, max_points, err)) return r == -3 ? ALEGO_ERR_CAPACITY : ALEGO_ERR_HIP;
  T.arc_frames_cap = max_frames; T.arc_points_cap = max_points;
  L = T;
  return 0;
}
static int map_stat(LmHost* lm, int slot, int* st4 /* [AS_W] */, std::string* err) {
  if (lm->L.arc_frames_cap <= 0) { *err = "the key-frame archive is off (alego_map_enable)"; return ALEGO_ERR_ARG; }
  return DevTry("map", err, "device read").wait(stream_of_slot(lm, slot)).down(st4, arc_stat_of(lm->L, slot), AS_W);
}
int lm_host_map_status(LmHost* lm, int slot, int* out4, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  out4[0] = st[AS_FRAMES]; out4[1] = st[AS_DROPPED]; out4[2] = st[AS_POINTS]; out4[3] = lm->L.arc_points_cap;
  return 0;
}
int lm_host_map_set_keyposes(LmHost* lm, int slot, int first, int n, const float* poses6, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  if (first < 0 || n < 0 || first > st[AS_FRAMES] || n > st[AS_FRAMES] - first || (n > 0 && !poses6)) { *err = "map_set_keyposes: range beyond the archived frames"; return ALEGO_ERR_ARG; }
  if (n == 0) return 0;
  // poses6 is [n][6]; the archive keeps KF_POSE_W floats per frame
  if (hipMemcpy2D(arc_pose_of(lm->L, slot, first), KF_POSE_W * sizeof(float), poses6, 6 * sizeof(float), 6 * sizeof(float), n,
                  hipMemcpyHostToDevice) != hipSuccess) { *err = "map_set_keyposes: copy failed"; return ALEGO_ERR_HIP; }
  return 0;
}
int lm_host_map_stamps(LmHost* lm, int slot, int first, int n, double* stamps, int write, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  if (first < 0 || n < 0 || first > st[AS_FRAMES] || n > st[AS_FRAMES] - first || (n > 0 && !stamps)) { *err = "map_stamps: range beyond the archived frames"; return ALEGO_ERR_ARG; }
  if (n == 0) return 0;
  double* dev = lm->L.arc_stamp + arc_row(lm->L, slot, first);
  DevTry c("map_stamps", err, "copy");
  if (write) c.up(dev, stamps, (size_t)n); else c.down(stamps, dev, (size_t)n);
  return c;
}
int lm_host_map_mark_stamped(LmHost* lm, int slot, hipStream_t st) {
  static const int one = 1;
  return lm->L.arc_frames_cap > 0 && dev_up(lm->L.arc_stamped + slot, &one, 1, st) != hipSuccess ? ALEGO_ERR_HIP : 0;
}
const LmCtx* lm_host_ctx(LmHost* lm) { return &lm->L; }

// ---- localisation mode (alego_loc_*; kernels_loc.hip) ----
// The map store: every frame transformed by its key pose and sorted by voxel key exactly as a ring entry is (lm_store_kf's re-transform path
// into kf_tmp_*, then the key-frame sort, VoxelGrid mode 1), once for the whole handle.  The rings of the slots are released: kfs_* / kf_raw_* /
// kf_cnt / kf_pose name the store from now on, and fr_stride = 0 sends every slot's frame f to row f of it.
// ---- what alego_loc_enable and alego_loc_enable_from_map share: the preconditions on the handle, the store and its view T, the undo, the swap of L
namespace {
// a fresh SLAM handle that may become a localising one (`what`: the call, for the messages)
int loc_handle_ready(LmHost* lm, const DevCtx& dfull, const std::string& what, std::string* err) {
  const LmCtx& L = lm->L;
  if (L.arc_frames_cap > 0 || L.pg_loops_cap > 0) { *err = what + ": the key-frame archive / key-pose graph belong to a mapping handle"; return ALEGO_ERR_ARG; }
  if (lm->comm) { *err = what + ": not available on a handle with a sharded registration (alego_dist_init)"; return ALEGO_ERR_ARG; }
  if (!dfull.opt_map_merge) { *err = what + ": ALEGO_MAP_MERGE=0 (concat + radix VoxelGrid) is a mapping-only path"; return ALEGO_ERR_ARG; }
  for (long f : lm->frames) if (f != 0) { *err = what + ": call it before the first scan of any slot"; return ALEGO_ERR_ARG; }
  if (int r = DevTry(what, err).wait(lm->st)) return r;
  return rings_empty(lm, what.c_str(), true, err);
}
// a frame of nc / ns / no points against the key-frame capacities of the handle
int loc_frame_fits(const LmCtx& L, const std::string& what, int i, int nc, int ns, int no, std::string* err) {
  if (nc <= L.kf_cap_c && ns <= L.kf_cap_s && no <= L.kf_cap_o) return 0;
  *err = what + ": frame " + std::to_string(i) + " (" + std::to_string(nc) + " corner, " + std::to_string(ns) + " surf, " + std::to_string(no) +
         " outlier points) exceeds the handle's key-frame capacities (" + std::to_string(L.kf_cap_c) + ", " + std::to_string(L.kf_cap_s) + ", " + std::to_string(L.kf_cap_o) + ")";
  return ALEGO_ERR_CAPACITY;
}
// The store of `rows` frames, n of them used, behind a view T of its own: the handle becomes a localising one — and its rings go (loc_store_commit) — only once
// every frame is in.  Until then any failure undoes the store (loc_store_undo) and leaves the handle the SLAM handle it was.
int loc_store_view(LmHost* lm, LmCtx* T, int rows, int n, double radius, const std::string& what, std::string* err) {
  *T = lm->L;
  const size_t F = (size_t)std::max(rows, 1);
  std::string aerr;
  if (!ring_alloc(lm, *T, F, &aerr)) {   // the handle stays what it was
    ring_release(lm, *T);
    *err = what + ": the map store of " + std::to_string(rows) + " frames does not fit (" + aerr + ")";
    return ALEGO_ERR_CAPACITY;
  }
  T->fr_stride = 0; T->fr_mod = (int)F; T->loc_on = 1; T->loc_n = n; T->loc_r2 = loc_r2(radius);
  return 0;
}
int loc_store_undo(LmHost* lm, LmCtx& T, int rc) {
  (void)dev_wait(lm->st[0]);
  ring_release(lm, T);
  return rc;
}
// The slots' rings give their memory back (no scan has used them).  The per-slot key-frame sort jobs in the job tables of vm[g] / vk[g]
// (lm_host_create) still name those rings: they run only for a slot whose LI_KF_PENDING is set, which lm_store_kf alone sets, and neither
// lm_store_kf nor a vk round is ever launched on a localising handle (launch_lm_register returns before it; retransform and
// lm_host_graph_apply sit behind API calls that refuse such a handle).
void loc_store_commit(LmHost* lm, const LmCtx& T) {
  ring_release(lm, lm->L);
  lm->L = T;
}
}  // namespace

int lm_host_loc_enable(LmHost* lm, const DevCtx& dfull, const alego_kf_in* frames, int n, double radius, std::string* err) {
  LmCtx& L = lm->L;
  const std::string what = "alego_loc_enable";
  if (L.loc_on) { *err = "alego_loc_enable: already enabled"; return ALEGO_ERR_ARG; }
  if (n < 0 || (n > 0 && !frames)) { *err = "alego_loc_enable: null frames / negative count"; return ALEGO_ERR_ARG; }
  if (int r = loc_handle_ready(lm, dfull, what, err)) return r;
  if (n > LOC_MAX_FRAMES) { *err = "alego_loc_enable: more than " + std::to_string(LOC_MAX_FRAMES) + " frames"; return ALEGO_ERR_CAPACITY; }
  for (int i = 0; i < n; ++i) {
    const alego_kf_in& f = frames[i];
    if (!kf_in_valid(f)) { *err = "alego_loc_enable: frame " + std::to_string(i) + ": null cloud / negative count"; return ALEGO_ERR_ARG; }
    if (int r = loc_frame_fits(L, what, i, f.n_corner, f.n_surf, f.n_outlier, err)) return r;
  }
  LmCtx T;
  if (int r = loc_store_view(lm, &T, n, n, radius, what, err)) return r;
  int* li0 = T.li;
  auto undo = [&](int rc) {
    (void)dev_wait(lm->st[0]);
    (void)hipMemset(li0 + LI_KF_PENDING, 0, 8 * sizeof(int));
    (void)hipMemset(li0 + LI_OVERFLOW, 0, sizeof(int));
    if (lm->vloc_made) { vox_destroy(&lm->vloc); lm->vloc_made = false; }
    return loc_store_undo(lm, T, rc);
  };
  // the sort jobs of slot 0's kf_tmp_*, with the store as their ring
  std::vector<VoxJob> jobs;
  kf_sort_jobs(T, lm->P, 0, &jobs);
  std::memset(&lm->vloc, 0, sizeof(VoxCtx));
  if (vox_create(&lm->vloc, jobs.data(), 2, err)) return undo(ALEGO_ERR_HIP);
  lm->vloc_made = true;
  lm->vloc.grid_small = 2; lm->vloc.grid_big = 2;
  hipStream_t st = lm->st[0];
  DevCtx d = dfull;
  d.slot0 = 0; d.n_launch = 1;
  DevTry c(what, err, "building the map store");
  for (int i = 0; i < n; ++i) {
    frame_to_row(T, kf_ring_row_at(T, 0, kf_entry(T, i), KF_CORNER), frames[i], &c);
    if (!c.ok()) break;
    launch_lm_retransform(d, T, kf_entry(T, i), st);   // row i of the store -> kf_tmp_* of slot 0
    if (int r = vox_run(lm->vloc, st, err)) return undo(r);
  }
  // slot 0 lent its key-frame staging words (LI_KF_PENDING .. LI_SORT_N1) to the build: it leaves as fresh as every other slot
  static_assert(LI_SORT_N1 - LI_KF_PENDING == 7 && LI_REBUILD_FB > LI_KF_PENDING && LI_MAP_PASS < LI_SORT_N1, "the words in between are zero on a fresh slot too");
  if (c.ok()) c.took(hipMemsetAsync(li0 + LI_KF_PENDING, 0, 8 * sizeof(int), st), "clearing");
  int ovf = 0;
  if (c.wait(st).at("device read").down(&ovf, li0 + LI_OVERFLOW, 1)) return undo(c);
  if (ovf) { *err = "alego_loc_enable: a frame was truncated while it was sorted"; return undo(ALEGO_ERR_CAPACITY); }
  loc_store_commit(lm, T);
  return 0;
}

// ---- the store from a slot's archive of a mapping handle, on the device (alego_loc_enable_from_map / alego_loc_update_from_map) ----
namespace {
// Staging + sort scratch of one chunk of the batched build stay within this many bytes: the chunk size is clamped to it (16x1800: 0.8 MB per
// frame, 128 frames fit; 64x2048: 5.7 MB per frame, 44 frames).
constexpr size_t LOC_BUILD_BUDGET = (size_t)256 << 20;
int loc_chunk_frames(const LmHost* lm, int n) {
  const LmCtx& L = lm->L;
  size_t per = 16 * ((size_t)L.kf_cap_c + L.total_cap) + LJ_W * sizeof(int);
  for (int cap : {L.kf_cap_c, L.total_cap}) if (cap > 8192) per += 20 * (size_t)cap;   // vox_create: key + two pair buffers for a job that can reach vox_big
  const long long fit = (long long)(LOC_BUILD_BUDGET / per);
  return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(std::max(lm->loc_chunk, 1), fit), std::max(n, 1)));
}
// the archive of `slot` of the source as it is now (its streams have been synchronised): frames stored, their arc_tab rows on the host
int loc_src_read(LmHost* src, int slot, const std::string& what, std::vector<int>* tab, std::string* err) {
  int st[AS_W];
  DevTry c(what, err);
  if (c.down(st, arc_stat_of(src->L, slot))) return c;
  const int n = std::max(0, std::min(st[AS_FRAMES], src->L.arc_frames_cap));   // (a source that dropped frames: the stored prefix is handed over)
  tab->assign((size_t)n * AT_W, 0);
  if (c.down(*tab, arc_tab_of(src->L, slot, 0))) return c;
  return n;
}
int loc_src_ok(LmHost* lm, LmHost* src, int slot, const std::string& what, std::string* err) {
  if (!src || src == lm) { *err = what + ": the source is a second handle, a mapping one"; return ALEGO_ERR_ARG; }
  if (src->L.arc_frames_cap <= 0) { *err = what + ": the source handle has no key-frame archive (alego_map_enable)"; return ALEGO_ERR_ARG; }
  if (slot < 0 || slot >= src->n_slots) { *err = what + ": slot out of range of the source handle"; return ALEGO_ERR_ARG; }
  return 0;
}
// Frames 0 .. n - 1 of S into rows 0 .. n - 1 of the store T names, in chunks: loc_fill, then one VoxelGrid round of the chunk's 2 C sort jobs, one workgroup
// per job.  Everything is queued on st and finished when this returns; tab: the host copy of the frames' arc_tab rows.
int loc_store_fill(LmHost* lm, const LmCtx& T, const KfArcSrc& S, const std::vector<int>& tab, int n, hipStream_t st, const std::string& what, std::string* err) {
  if (n == 0) return dev_wait(st) == hipSuccess ? 0 : ALEGO_ERR_HIP;
  const int C = loc_chunk_frames(lm, n);
  DevPool tmp;
  float4 *stage_c = nullptr, *stage_s = nullptr;
  int* words = nullptr;   // [C][LJ_W], then the overflow word of all jobs
  if (tmp.get(&stage_c, (size_t)C * T.kf_cap_c, false) != hipSuccess || tmp.get(&stage_s, (size_t)C * T.total_cap, false) != hipSuccess ||
      tmp.get(&words, (size_t)C * LJ_W + 1, true) != hipSuccess) { *err = what + ": the staging area of " + std::to_string(C) + " frames does not fit"; return ALEGO_ERR_HIP; }
  int* ovf = words + (size_t)C * LJ_W;
  std::vector<VoxJob> jobs;
  for (int j = 0; j < C; ++j) {
    int* w = words + (size_t)j * LJ_W;
    static_assert(LJ_N_S == LJ_N_C + 1 && LJ_SORT_N1 == LJ_SORT_N + 1, "kf_sort_job_pair reads / writes the counts as pairs");
    kf_sort_job_pair(T, lm->P, 0, stage_c + (size_t)j * T.kf_cap_c, stage_s + (size_t)j * T.total_cap, w + LJ_N_C, w + LJ_SORT_N, w + LJ_ENABLE, w + LJ_ROW, ovf, &jobs);
  }
  VoxCtx V;
  if (vox_create(&V, jobs.data(), (int)jobs.size(), err)) return ALEGO_ERR_HIP;   // (grid_small = grid_big = the job count: one job per workgroup across the chip)
  int rc = 0;
  for (int f0 = 0; f0 < n && !rc; f0 += C) {
    int n_max = 0;
    for (int f = f0; f < std::min(n, f0 + C); ++f) for (int k = 0; k < KF_KINDS; ++k) n_max = std::max(n_max, tab[(size_t)f * AT_W + AT_N + k]);
    launch_loc_fill(T, S, f0, n, C, n_max, stage_c, stage_s, words, st);
    rc = vox_run(V, st, err);
  }
  int o = 0;
  const hipError_t e = dev_wait(st);
  if (!rc) rc = DevTry(what, err).took(e, "building the map store").down(&o, ovf, 1);
  if (!rc && o) { *err = what + ": a frame was truncated while it was sorted"; rc = ALEGO_ERR_CAPACITY; }
  vox_destroy(&V);
  tmp.clear();
  return rc;
}
}  // namespace

int lm_host_loc_enable_from_map(LmHost* lm, const DevCtx& dfull, LmHost* src, int slot, double radius, int capacity, std::string* err) {
  const std::string what = "alego_loc_enable_from_map";
  LmCtx& L = lm->L;
  if (L.loc_on) { *err = what + ": already enabled"; return ALEGO_ERR_ARG; }
  if (int r = loc_src_ok(lm, src, slot, what, err)) return r;
  if (int r = loc_handle_ready(lm, dfull, what, err)) return r;
  std::vector<int> tab;
  const int n = loc_src_read(src, slot, what, &tab, err);
  if (n < 0) return n;
  if (n > LOC_MAX_FRAMES) { *err = what + ": more than " + std::to_string(LOC_MAX_FRAMES) + " frames"; return ALEGO_ERR_CAPACITY; }
  if (capacity <= 0) capacity = n;
  if (capacity < n || capacity > LOC_MAX_FRAMES) {
    *err = what + ": capacity " + std::to_string(capacity) + " is not within the " + std::to_string(n) + " archived frames .. " + std::to_string(LOC_MAX_FRAMES);
    return ALEGO_ERR_CAPACITY;
  }
  for (int i = 0; i < n; ++i) if (int r = loc_frame_fits(L, what, i, tab[(size_t)i * AT_W + AT_N + KF_CORNER], tab[(size_t)i * AT_W + AT_N + KF_SURF], tab[(size_t)i * AT_W + AT_N + KF_OUTL], err)) return r;
  LmCtx T;
  if (int r = loc_store_view(lm, &T, capacity, n, radius, what, err)) return r;
  if (int r = loc_store_fill(lm, T, kf_arc_src(src->L, slot), tab, n, lm->st[0], what, err)) return loc_store_undo(lm, T, r);
  loc_store_commit(lm, T);
  return 0;
}

int lm_host_loc_update_from_map(LmHost* lm, LmHost* src, int slot, bool* rewritten, std::string* err) {
  const std::string what = "alego_loc_update_from_map";
  *rewritten = false;
  LmCtx& L = lm->L;
  if (!L.loc_on) { *err = what + ": the handle does not localise (alego_loc_enable / alego_loc_enable_from_map)"; return ALEGO_ERR_ARG; }
  if (int r = loc_src_ok(lm, src, slot, what, err)) return r;
  if (int r = DevTry(what, err).wait(lm->st)) return r;
  std::vector<int> tab;
  const int n = loc_src_read(src, slot, what, &tab, err);
  if (n < 0) return n;
  if (n > L.fr_mod) { *err = what + ": " + std::to_string(n) + " archived frames exceed the store's capacity of " + std::to_string(L.fr_mod); return ALEGO_ERR_CAPACITY; }
  for (int i = 0; i < n; ++i) if (int r = loc_frame_fits(L, what, i, tab[(size_t)i * AT_W + AT_N + KF_CORNER], tab[(size_t)i * AT_W + AT_N + KF_SURF], tab[(size_t)i * AT_W + AT_N + KF_OUTL], err)) return r;
  // From here on the store is rewritten.  Counts, poses, run counts and boxes start from zero as in a fresh store (an empty run writes no box; rows
  // beyond the new frames name nothing); points beyond a row's counts are never read.
  hipStream_t st = lm->st[0];
  const size_t F = (size_t)L.fr_mod;
  *rewritten = true;
  hipError_t e = hipMemsetAsync(L.kfs_n, 0, 2 * F * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(L.kfs_box, 0, 2 * F * 8 * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(kf_cnt_of(L, 0), 0, F * KF_CNT_W * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(kf_pose_of(L, 0), 0, F * KF_POSE_W * sizeof(float), st);
  int rc = e == hipSuccess ? 0 : ALEGO_ERR_HIP;
  if (rc) *err = what + ": " + hipGetErrorString(e);
  if (!rc) rc = loc_store_fill(lm, L, kf_arc_src(src->L, slot), tab, n, st, what, err);
  L.loc_n = rc ? 0 : n;   // a failure in the middle leaves the store empty: every slot is off the map and dead-reckons
  launch_loc_reset_windows(L, lm->n_slots, st);
  const hipError_t we = dev_wait(st);
  if (!rc && (rc = DevTry(what, err).took(we, "the window reset"))) L.loc_n = 0;
  return rc;
}
int lm_host_set_loc_chunk(LmHost* lm, int frames) { lm->loc_chunk = std::max(1, frames); return 0; }
int lm_host_loc_status(LmHost* lm, int slot, int* out4, std::string* err) {
  const LmCtx& L = lm->L;
  if (!L.loc_on) { *err = "alego_loc_status: the handle does not localise (alego_loc_enable)"; return ALEGO_ERR_ARG; }
  int li[LI_COUNT];
  if (int r = DevTry("alego_loc_status", err, "device read").wait(stream_of_slot(lm, slot)).down(li, L.li + (size_t)slot * LI_COUNT)) return r;
  out4[0] = L.loc_n; out4[1] = li[LI_REC_CNT]; out4[2] = li[LI_NREBUILD]; out4[3] = li[LI_OPTIMIZED];
  return 0;
}
bool lm_host_localising(LmHost* lm) { return lm->L.loc_on != 0; }

// ---- the key-pose graph (alego_graph_*) ----
int lm_host_graph_enable(LmHost* lm, int max_loops, const double* odom_var6, std::string* err) {
  LmCtx& L = lm->L;
  if (max_loops < 1 || max_loops > ALEGO_GRAPH_MAX_LOOPS) { *err = "graph_enable: max_loops out of range"; return ALEGO_ERR_ARG; }
  static const double dflt[6] = {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6};   // laserMapping.cpp:68-70
  const double* v = odom_var6 ? odom_var6 : dflt;
  for (int k = 0; k < 6; ++k) if (!(v[k] > 0.0) || !(v[k] < 1e300)) { *err = "graph_enable: variances must be positive and finite"; return ALEGO_ERR_ARG; }
  if (int r = rings_empty(lm, "graph_enable", false, err)) return r;   // the chain starts with the prior on frame 0: the graph has to exist before the first key frame
  const size_t B = lm->n_slots, F = L.arc_frames_cap;
  LmCtx T = L;
  bool ok = A(lm, &T.pg_chain, B * F, err) && A(lm, &T.pg_loops, B * max_loops, err) && A(lm, &T.pg_corr, B * 16, err) && A(lm, &T.pg_stat, B * PS_W, err) &&
            A(lm, &T.pg_est, B * F * 12, err);
  if (!ok) return ALEGO_ERR_HIP;
  for (int k = 0; k < 6; ++k) T.pg_odom_var[k] = v[k];
  T.pg_loops_cap = max_loops;
  L = T;
  return 0;
}

// ---- the two opt-in siblings of the registration: its covariance (alego_regcov_*; lm_regcov in kernels_lm.hip) and solution remapping (alego_remap_*; lm_solve_remap) ----
// What both *_enable calls refuse, in the order they refuse it: on twice, a sharded handle, bad_options (the feature's own refusal of its options, or
// null: it comes before the state of the slots), a scan that has reached LaserMapping, a ring that is not empty.
static int lm_feature_preconditions(LmHost* lm, const char* what, bool on, const char* bad_options, std::string* err) {
  if (on) { *err = std::string(what) + ": already enabled"; return ALEGO_ERR_ARG; }
  if (lm->comm || lm->L.shard_world > 0) { *err = std::string(what) + ": not available on a handle with a sharded registration (alego_dist_init)"; return ALEGO_ERR_ARG; }
  if (bad_options) { *err = bad_options; return ALEGO_ERR_ARG; }
  for (long f : lm->frames) if (f != 0) { *err = std::string(what) + ": call it before the first scan reaches LaserMapping"; return ALEGO_ERR_ARG; }
  return rings_empty(lm, what, true, err);
}
// What both *_get calls do — one copy: the records of slots [lo, hi] of the list, picked apart on the host.  what: the call, enable: the call that turns it on.
template <class Rec> static int lm_records_get(LmHost* lm, const char* what, const char* enable, bool on, const Rec* dev_records, const int* slots, int n, Rec* out, std::string* err) {
  if (!on) { *err = std::string(what) + ": the feature is off (" + enable + ")"; return ALEGO_ERR_ARG; }
  if (int r = gate_slot_list(what, slots, n, lm->n_slots, true, err)) return r;
  if (n == 0) return 0;
  const int lo = *std::min_element(slots, slots + n), hi = *std::max_element(slots, slots + n);
  std::vector<Rec> tmp((size_t)(hi - lo + 1));
  if (int r = DevTry(what, err).wait(lm->st).down(tmp, dev_records + lo)) return r;
  for (int i = 0; i < n; ++i) out[i] = tmp[(size_t)(slots[i] - lo)];
  return 0;
}

static const double kOdomVarDefault[6] = {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6};   // laserMapping.cpp:68-70, the default of lm_host_graph_enable
bool lm_host_regcov_opts(LmHost* lm, double* opt16) {
  if (lm && lm->rc_on) { std::memcpy(opt16, lm->rc_opt, sizeof(lm->rc_opt)); return true; }
  (void)rc_resolve(nullptr, kOdomVarDefault, opt16);
  return false;
}
int lm_host_regcov_enable(LmHost* lm, const alego_regcov_opts* opts, std::string* err) {
  static_assert(offsetof(alego_regcov_opts, graph) == RC_OPT_W * sizeof(double), "rc_resolve reads the options' doubles in the RC_* order");
  LmCtx& L = lm->L;
  const bool graph = opts && opts->graph != 0;
  double opt[RC_OPT_W];
  const char* bad = graph && L.pg_loops_cap <= 0 ? "alego_regcov_enable: graph = 1 needs the key-pose graph (alego_graph_enable first)"
                    : rc_resolve(opts ? &opts->sigma0 : nullptr, L.pg_loops_cap > 0 ? L.pg_odom_var : kOdomVarDefault, opt) ? "alego_regcov_enable: an option is not finite, or var_min exceeds var_max" : nullptr;
  if (int r = lm_feature_preconditions(lm, "alego_regcov_enable", lm->rc_on, bad, err)) return r;
  LmCtx T = L;
  double* dopt = nullptr;
  if (!A(lm, &T.rc_rec, (size_t)lm->n_slots, err) || !A(lm, &dopt, (size_t)RC_OPT_W, err)) return ALEGO_ERR_HIP;
  if (int r = DevTry("alego_regcov_enable", err, "copy").up(dopt, opt)) return r;
  T.rc_opt = dopt; T.rc_graph = graph ? 1 : 0;
  L = T;
  std::memcpy(lm->rc_opt, opt, sizeof(opt));
  lm->rc_on = true;
  return 0;
}
int lm_host_regcov_get(LmHost* lm, const int* slots, int n, alego_regcov* out, std::string* err) {
  return lm_records_get(lm, "alego_regcov_get", "alego_regcov_enable", lm->rc_on, lm->L.rc_rec, slots, n, out, err);
}
bool lm_host_regcov_on(LmHost* lm) { return lm->rc_on; }

double lm_host_remap_eig_min(LmHost* lm) { return lm && lm->rm_on ? lm->L.rm_eig_min : RC_DEFAULT_EIG_MIN; }
int lm_host_remap_enable(LmHost* lm, const alego_remap_opts* opts, std::string* err) {
  LmCtx& L = lm->L;
  double eig_min;
  const char* bad = rm_resolve(opts ? &opts->eig_min : nullptr, &eig_min) ? "alego_remap_enable: eig_min is not finite" : nullptr;
  if (int r = lm_feature_preconditions(lm, "alego_remap_enable", lm->rm_on, bad, err)) return r;
  LmCtx T = L;
  if (!A(lm, &T.rm_rec, (size_t)lm->n_slots, err)) return ALEGO_ERR_HIP;
  T.rm_eig_min = eig_min;
  L = T;
  lm->rm_on = true;
  return 0;
}
int lm_host_remap_get(LmHost* lm, const int* slots, int n, alego_remap* out, std::string* err) {
  return lm_records_get(lm, "alego_remap_get", "alego_remap_enable", lm->rm_on, lm->L.rm_rec, slots, n, out, err);
}

// Frames of the slots with mask[slot] != 0 (mask_dev: the same words on the device) go through kf_tmp_* and the key-frame sort jobs, oldest first, one
// frame of every such slot of a stream group per round (what alego_lm_set_keypose does for one frame of one slot); retransform(slot0, n, j, stream)
// launches round j for the group's slots.  all: after the flush every slot of the group is noted as sorted (as map_update notes it), not only the masked.
template <class F> static int resort_rounds(LmHost* lm, const std::vector<int>& mask, const int* mask_dev, int rounds, int all, F retransform, const char* what, std::string* err) {
  const LmCtx& L = lm->L;
  for (size_t g = 0; g < lm->st.size(); ++g) {
    const int s0 = (int)g * lm->gsize, n = std::min(lm->gsize, lm->n_slots - s0);
    bool any = false;
    for (int s = s0; s < s0 + n; ++s) any = any || mask[s];
    if (!any) continue;
    hipStream_t st = lm->st[g];
    // a key frame saved by the last mapping frame may still wait in kf_tmp_* for its sort: flush it before the buffer is reused
    if (int r = vox_run(lm->vk[g], st, err)) return r;
    launch_pg_sorted(L, mask_dev, s0, n, all, st);
    for (int j = 0; j < rounds; ++j) {
      retransform(s0, n, j, st);
      if (int r = vox_run(lm->vk[g], st, err)) return r;
      launch_pg_sorted(L, mask_dev, s0, n, 0, st);
    }
  }
  return DevTry(what, err, "key-frame transform").wait(lm->st);
}

int lm_host_graph_apply(LmHost* lm, const std::vector<int>& apply, const int* apply_dev, int n_poses_max, std::string* err) {
  const LmCtx& L = lm->L;
  DevTry c("graph apply", err);
  if (c.wait(lm->st)) return c;
  launch_pg_apply(L, apply_dev, lm->n_slots, lm->st[0]);
  if (c.at("pose write").wait(lm->st[0])) return c;
  // every resident frame of every applied slot
  return resort_rounds(lm, apply, apply_dev, std::min(L.K, n_poses_max), 1,
                       [&](int s0, int n, int j, hipStream_t st) { launch_pg_retransform(L, apply_dev, s0, n, j, st); }, "graph apply", err);
}

// ---- a slot moved, one archive appended to another's (alego_map_move / alego_map_merge; kernels_merge.hip) ----
namespace {
// the per-slot words `tail` (frames to re-sort, newest last) on the device, then the rounds
int merge_rounds(LmHost* lm, const std::vector<int>& tail, const char* what, std::string* err) {
  const LmCtx& L = lm->L;
  if (int r = DevTry(what, err, "upload").took(lm->mg_tail.reserve(tail.size())).up(lm->mg_tail.p, tail)) return r;
  const int* dev = lm->mg_tail.p;
  return resort_rounds(lm, tail, dev, *std::max_element(tail.begin(), tail.end()), 0,
                       [&](int s0, int n, int j, hipStream_t st) { launch_mg_retransform(L, dev, s0, n, j, st); }, what, err);
}
int read_stats(LmHost* lm, std::vector<int>* arc, std::vector<int>* pg, const char* what, std::string* err) {
  const LmCtx& L = lm->L;
  DevTry c(what, err);
  if (c.wait(lm->st)) return c;
  arc->assign((size_t)lm->n_slots * AS_W, 0); pg->assign((size_t)lm->n_slots * PS_W, 0);
  c.down(*arc, L.arc_stat);
  if (L.pg_loops_cap > 0) c.down(*pg, L.pg_stat);
  return c;
}
}  // namespace

int lm_host_map_move(LmHost* lm, const int* slots, int n, const double* T12, int* out_status, std::string* err) {
  const LmCtx& L = lm->L;
  std::vector<int> arc, pg;
  if (int r = read_stats(lm, &arc, &pg, "map_move", err)) return r;
  std::vector<MgMove> mv;
  std::vector<int> tail((size_t)lm->n_slots, 0);
  for (int i = 0; i < n; ++i) {
    const int* st = arc.data() + (size_t)slots[i] * AS_W;
    out_status[i] = st[AS_DROPPED] ? -1 : (st[AS_FRAMES] == 0 ? 0 : 2);
    if (out_status[i] != 2) continue;
    MgMove m{slots[i], st[AS_FRAMES], 0, 0, {}};
    std::memcpy(m.T, T12 + (size_t)i * 12, sizeof(m.T));
    mv.push_back(m);
    tail[slots[i]] = std::min(L.K, st[AS_FRAMES]);   // the resident frames, as alego_lm_set_keypose accepts them
  }
  if (mv.empty()) return 0;
  DevTry c("map_move", err, "upload");
  if (c.took(lm->mg_moves.reserve(mv.size())).up(lm->mg_moves.p, mv)) return c;
  launch_mg_move(L, lm->mg_moves.p, (int)mv.size(), lm->st[0]);
  if (c.at("pose write").wait(lm->st[0])) return c;
  return merge_rounds(lm, tail, "map_move", err);
}

int lm_host_map_merge(LmHost* lm, PgCtx** pc, const int* src, const int* dst, int n, const double* T12, double stamp_off, const double* seam_var6,
                      const alego_map_align_hyp* hyp, alego_map_merge_result* out, std::string* err) {
  const LmCtx& L = lm->L;
  const bool graph = L.pg_loops_cap > 0;
  std::vector<int> arc, pg;
  if (int r = read_stats(lm, &arc, &pg, "map_merge", err)) return r;
  // ---- the plan: every count is known now, so every check comes before anything is written
  std::vector<MgPair> pairs;
  std::vector<int2> items;
  std::vector<PgAppend> edges;
  std::vector<int> tail((size_t)lm->n_slots, 0);
  int ns_max = 0, tail_max = 0;
  for (int i = 0; i < n; ++i) {
    const int *as = arc.data() + (size_t)src[i] * AS_W, *ad = arc.data() + (size_t)dst[i] * AS_W;
    const int ns = as[AS_FRAMES], nd = ad[AS_FRAMES], ps = as[AS_POINTS], pd = ad[AS_POINTS];
    alego_map_merge_result& o = out[i];
    o = alego_map_merge_result{0, 0, 0, 0, 0};
    if (as[AS_DROPPED] || ad[AS_DROPPED]) { o.status = -1; continue; }
    if (ns == 0) continue;
    const int ls = graph ? pg[(size_t)src[i] * PS_W + PS_LOOPS] : 0, ld = graph ? pg[(size_t)dst[i] * PS_W + PS_LOOPS] : 0;
    int nx = 0;
    if (graph && hyp) for (int q = 0; q < ALEGO_ALIGN_MAX_QUERIES; ++q) { const alego_map_align_hyp& x = hyp[(size_t)i * ALEGO_ALIGN_MAX_QUERIES + q]; nx += (x.accepted && x.inlier) ? 1 : 0; }
    if ((long long)nd + ns > L.arc_frames_cap || (long long)pd + ps > L.arc_points_cap || ld + ls + nx > L.pg_loops_cap) { o.status = -3; continue; }
    if (graph && ls + nx > 0) {
      std::vector<alego_graph_edge> sl((size_t)ls);
      std::vector<float> kp((size_t)(nx ? nd : 0) * KF_POSE_W);
      if (int r = DevTry("map_merge", err).down(sl, L.pg_loops + (size_t)src[i] * L.pg_loops_cap).down(kp, arc_pose_of(L, dst[i], 0))) return r;
      PgAppend a;
      std::memset(&a, 0, sizeof(a));
      a.slot = dst[i];
      for (int k = 0; k < 16; ++k) a.corr[k] = k % 5 == 0 ? 1.f : 0.f;   // alego_graph_add_edge(dst, e, NULL)
      for (int l = 0; l < ls; ++l) { mg_shift_edge(&sl[l], nd, &a.e); edges.push_back(a); }
      for (int q = 0; q < ALEGO_ALIGN_MAX_QUERIES && nx; ++q) {
        const alego_map_align_hyp& x = hyp[(size_t)i * ALEGO_ALIGN_MAX_QUERIES + q];
        if (!(x.accepted && x.inlier)) continue;
        if (x.src_frame < 0 || x.src_frame >= ns || x.dst_frame < 0 || x.dst_frame >= nd) { *err = "map_merge: an inlier hypothesis names a frame outside the pair's archives"; return ALEGO_ERR_ARG; }
        if (alego_map_align_edge(&x, kp.data() + (size_t)x.dst_frame * KF_POSE_W, nd, &a.e) != ALEGO_OK) { *err = "map_merge: a hypothesis gives no edge"; return ALEGO_ERR_ARG; }
        const double v = a.e.variance[0];
        bool fin = v > 0.0 && v - v == 0.0;
        for (int k = 0; k < 12; ++k) fin = fin && a.e.between[k] - a.e.between[k] == 0.0;
        if (!fin) { *err = "map_merge: an inlier hypothesis has a fitness that is not positive and finite, or a measurement that is not finite"; return ALEGO_ERR_ARG; }
        edges.push_back(a);
      }
    }
    o = alego_map_merge_result{2, ns, ps, ls, nx};
    MgPair P;
    std::memset(&P, 0, sizeof(P));
    P.src = src[i]; P.dst = dst[i]; P.ns = ns; P.nd = nd; P.ps = ps; P.pd = pd; P.tail = std::min(ns, L.KR);
    std::memcpy(P.T, T12 + (size_t)i * 12, sizeof(P.T));
    P.stamp_off = stamp_off;
    for (int k = 0; k < 6; ++k) P.seam_var[k] = seam_var6 ? seam_var6[k] : L.pg_odom_var[k];
    for (int it = 0; it * MG_ITEM < ps; ++it) items.push_back(make_int2((int)pairs.size(), it));
    pairs.push_back(P);
    tail[dst[i]] = P.tail;
    ns_max = std::max(ns_max, ns); tail_max = std::max(tail_max, P.tail);
  }
  if (pairs.empty()) return 0;
  // ---- points, rows and edges, ring rows: three launches for all pairs
  hipStream_t st = lm->st[0];
  DevTry c("map_merge", err, "upload");
  c.took(lm->mg_pairs.reserve(pairs.size())).took(lm->mg_items.reserve(std::max<size_t>(items.size(), 1)));
  if (c.up(lm->mg_pairs.p, pairs).up(lm->mg_items.p, items)) return c;
  launch_mg_copy(L, lm->mg_pairs.p, lm->mg_items.p, (int)items.size(), st);
  launch_mg_frames(L, lm->mg_pairs.p, (int)pairs.size(), ns_max, st);
  launch_mg_ring(L, lm->mg_pairs.p, (int)pairs.size(), tail_max, st);
  if (c.at("append").wait(st)) return c;
  // ---- every ring row that now holds a source frame is transformed and sorted, oldest first
  if (int r = merge_rounds(lm, tail, "map_merge", err)) return r;
  return graph ? graph_append(pc, L, lm->n_slots, edges, st, err) : 0;
}
// ---- a slot's archive thinned in place (alego_map_thin / alego_debug_thin_select; kernels_thin.hip) ----
namespace {
// th_select for `jobs` (pose, tab, pose_stride, n, slot, r2 set by the caller): the tables are laid out in th_ints / th_prot, the counts of
// every job come back in cnt[job][4] = N', P', the first dropped id, the point offset there
int thin_select(LmHost* lm, std::vector<ThJob>& jobs, std::vector<int>* cnt, const char* what, std::string* err) {
  const size_t nj = jobs.size();
  size_t ints = 4 * nj, prot = 0;
  for (const ThJob& J : jobs) { ints += 3 * (size_t)J.n + 1; prot += (size_t)J.n; }
  if (lm->th_jobs.reserve(nj) != hipSuccess || lm->th_ints.reserve(ints) != hipSuccess || lm->th_prot.reserve(std::max<size_t>(prot, 1)) != hipSuccess) { *err = std::string(what) + ": allocation failed"; return ALEGO_ERR_HIP; }
  size_t io = 4 * nj, po = 0;
  for (size_t w = 0; w < nj; ++w) {
    ThJob& J = jobs[w];
    J.cnt = lm->th_ints.p + 4 * w;
    J.new_id = lm->th_ints.p + io; J.old_id = J.new_id + J.n; J.new_off = J.old_id + J.n;
    J.protect = lm->th_prot.p + po;
    io += 3 * (size_t)J.n + 1; po += (size_t)J.n;
  }
  hipStream_t st = lm->st[0];
  cnt->assign(4 * nj, 0);
  DevTry c(what, err);
  if (c.up(lm->th_jobs.p, jobs)) return c;
  launch_th_select(lm->L, lm->th_jobs.p, (int)nj, st);
  return c.at("the selection").wait(st).down(*cnt, lm->th_ints.p);
}
}  // namespace

int lm_host_map_thin(LmHost* lm, const int* slots, int n, double min_dist, alego_map_thin_result* out, int* first_dropped, std::string* err) {
  const LmCtx& L = lm->L;
  const bool graph = L.pg_loops_cap > 0;
  std::vector<int> arc, pg;
  if (int r = read_stats(lm, &arc, &pg, "map_thin", err)) return r;
  std::vector<ThJob> jobs;
  std::vector<int> who;
  for (int i = 0; i < n; ++i) {
    const int* as = arc.data() + (size_t)slots[i] * AS_W;
    out[i] = alego_map_thin_result{0, as[AS_FRAMES], as[AS_FRAMES], as[AS_POINTS], as[AS_POINTS]};
    first_dropped[i] = as[AS_FRAMES];
    if (as[AS_DROPPED]) { out[i].status = -1; continue; }
    if (as[AS_FRAMES] == 0) continue;
    out[i].status = 1;
    ThJob J;
    std::memset(&J, 0, sizeof(J));
    J.pose = arc_pose_of(L, slots[i], 0); J.pose_stride = KF_POSE_W; J.tab = arc_tab_of(L, slots[i], 0);
    J.n = as[AS_FRAMES]; J.slot = slots[i]; J.r2 = th_r2(min_dist);
    jobs.push_back(J); who.push_back(i);
  }
  if (jobs.empty()) return 0;
  std::vector<int> cnt;
  if (int r = thin_select(lm, jobs, &cnt, "map_thin", err)) return r;
  // ---- every size is known now: the slots that drop a frame, their copy items, their places in the staging buffers
  std::vector<ThJob> go;
  std::vector<MgPair> ring;
  std::vector<int2> items;
  std::vector<int> tail((size_t)lm->n_slots, 0);
  int rows_max = 0, lanes_max = 1, tail_max = 0, stage_pt = 0, stage_row = 0;
  for (size_t w = 0; w < jobs.size(); ++w) {
    ThJob J = jobs[w];
    const int* c = cnt.data() + 4 * w;
    if (c[0] == J.n) continue;   // nothing to drop: the slot stays byte-unchanged
    alego_map_thin_result& o = out[who[w]];
    o.status = 2; o.frames = c[0]; o.points = c[1];
    first_dropped[who[w]] = c[2];
    J.n_new = c[0]; J.p_new = c[1]; J.first = c[2]; J.p0 = c[3];
    J.n_loops = graph ? pg[(size_t)J.slot * PS_W + PS_LOOPS] : 0;
    J.stage_pt = stage_pt; J.stage_row = stage_row;
    stage_pt += J.p_new - J.p0; stage_row += J.n_new - J.first;
    for (int it = 0; it * MG_ITEM < J.p_new - J.p0; ++it) items.push_back(make_int2((int)go.size(), it));
    rows_max = std::max(rows_max, J.n_new - J.first); lanes_max = std::max(lanes_max, std::max(J.n_new - J.first, J.n_loops));
    MgPair P;   // mg_ring reading the slot's own archive: "source" frames 0 .. N' - 1 behind an empty destination
    std::memset(&P, 0, sizeof(P));
    P.src = J.slot; P.dst = J.slot; P.ns = J.n_new; P.nd = 0; P.tail = std::min(J.n_new, L.KR);
    ring.push_back(P);
    tail[J.slot] = P.tail; tail_max = std::max(tail_max, P.tail);
    go.push_back(J);
  }
  if (go.empty()) return 0;
  hipStream_t st = lm->st[0];
  if (lm->th_items.reserve(std::max<size_t>(items.size(), 1)) != hipSuccess || lm->th_pts.reserve(std::max(stage_pt, 1)) != hipSuccess ||
      lm->th_rows.reserve(std::max(stage_row, 1)) != hipSuccess || lm->mg_pairs.reserve(ring.size()) != hipSuccess) { *err = "map_thin: allocation failed"; return ALEGO_ERR_HIP; }
  DevTry c("map_thin", err);
  if (c.up(lm->th_jobs.p, go).up(lm->mg_pairs.p, ring).up(lm->th_items.p, items)) return c;
  // ---- points and rows through the staging buffers (each read launch ends before its write launch starts), then the ring rows
  launch_th_gather(L, lm->th_jobs.p, lm->th_items.p, (int)items.size(), lm->th_pts.p, st);
  launch_th_rows_read(L, lm->th_jobs.p, (int)go.size(), rows_max, lm->th_rows.p, st);
  launch_th_scatter(L, lm->th_jobs.p, lm->th_items.p, (int)items.size(), lm->th_pts.p, st);
  launch_th_rows_write(L, lm->th_jobs.p, (int)go.size(), lanes_max, lm->th_rows.p, st);
  launch_mg_ring(L, lm->mg_pairs.p, (int)ring.size(), tail_max, st);
  if (c.at("compaction").wait(st)) return c;
  return merge_rounds(lm, tail, "map_thin", err);
}

int lm_host_debug_thin_select(LmHost* lm, const float* keyposes6, const uint8_t* protect, int n, double min_dist, uint8_t* keep, std::string* err) {
  if (n == 0) return 0;
  DevTry c("debug_thin_select", err, "upload");
  if (c.took(lm->th_pose.reserve((size_t)n * 6)).up(lm->th_pose.p, keyposes6, (size_t)n * 6)) return c;
  std::vector<ThJob> jobs(1);
  std::memset(&jobs[0], 0, sizeof(ThJob));
  jobs[0].pose = lm->th_pose.p; jobs[0].pose_stride = 6; jobs[0].n = n; jobs[0].slot = -1; jobs[0].r2 = th_r2(min_dist);
  // (the tables are laid out first, so that the caller's protect mask can go to its place before the launch)
  if (c.took(lm->th_prot.reserve((size_t)n)).up(lm->th_prot.p, protect, (size_t)n)) return c;
  std::vector<int> cnt;
  if (int r = thin_select(lm, jobs, &cnt, "debug_thin_select", err)) return r;
  std::vector<int> id((size_t)n);
  if (c.at("device read").down(id, jobs[0].new_id)) return c;
  for (int i = 0; i < n; ++i) keep[i] = id[i] >= 0 ? 1 : 0;
  return cnt[0];
}
int lm_host_map_get_keyframe(LmHost* lm, int slot, int id, alego_keyframe* out, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  if (id < 0 || id >= st[AS_FRAMES]) { *err = "map_get_keyframe: frame not archived"; return ALEGO_ERR_ARG; }
  int tab[AT_W];
  if (int r = DevTry("map_get_keyframe", err, "copy").down(tab, arc_tab_of(lm->L, slot, id))) return r;
  const KfArcFrame A = kf_arc_frame(lm->L, slot, id, tab);
  const float4* const src[KF_KINDS] = {A.pts, A.pts + A.nc, A.pts + A.nc + A.ns};
  return frame_to_host("map_get_keyframe", id, A.pose, tab + AT_N, src, out, err);
}
// the filtered (gv.out) or raw (gv.in) cloud of `n` points to the caller: count only, capacity error, or copy
static int copy_out(const float4* src, int n, alego_point* out, int cap, const char* what, std::string* err) {
  if (!out && cap == 0) return n;
  if (cap < n || (n > 0 && !out)) { *err = std::string(what) + ": output capacity"; return ALEGO_ERR_CAPACITY; }
  if (int r = DevTry(what, err, "copy").down(out, src, (size_t)std::max(n, 0))) return r;
  return n;
}
// the cloud the launches on `s` leave in gv.in, its size in gv.cnt[0], to the caller: as it is (leaf <= 0) or through the device-wide VoxelGrid
static int assembled_out(LmHost* lm, hipStream_t s, float leaf, alego_point* out, int cap, const char* what, std::string* err) {
  GvCtx& G = lm->gv;
  int n = 0;
  DevTry c(what, err, "assembly");
  if (c.wait(s).down(&n, G.cnt, 1)) return c;
  if (leaf <= 0.f) return copy_out(G.in, n, out, cap, what, err);
  if (int r = gv_filter(&G, n, leaf, s, err)) return r == -3 ? ALEGO_ERR_CAPACITY : ALEGO_ERR_HIP;
  int m = 0;
  if (c.at("VoxelGrid").wait(s).down(&m, G.cnt + 1, 1)) return c;
  return copy_out(G.out, m, out, cap, what, err);
}
int lm_host_map_assemble(LmHost* lm, int slot, int kinds, float leaf, alego_point* out, int cap, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  if ((kinds & ~15) || !(kinds & 7) || cap < 0) { *err = "map_assemble: kinds must select surf / corner / outlier (optionally | FRAME_ID)"; return ALEGO_ERR_ARG; }
  hipStream_t s = stream_of_slot(lm, slot);
  GvCtx& G = lm->gv;
  if (int r = gv_reserve(&G, lm->L.arc_points_cap, err)) return r == -3 ? ALEGO_ERR_CAPACITY : ALEGO_ERR_HIP;
  launch_map_assemble(lm->L, slot, st[AS_FRAMES], kinds, G.in, lm->arc_off, G.cnt, s);
  return assembled_out(lm, s, leaf, out, cap, "map_assemble", err);
}
int lm_host_map_keyposes(LmHost* lm, int slot, alego_point* out, int cap, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  const int nf = st[AS_FRAMES];
  if (!out && cap == 0) return nf;
  if (cap < nf || (nf > 0 && !out)) { *err = "map_keyposes: output capacity"; return ALEGO_ERR_CAPACITY; }
  std::vector<float> kp((size_t)nf * KF_POSE_W);
  if (int r = DevTry("map_keyposes", err, "copy").down(kp, arc_pose_of(lm->L, slot, 0))) return r;
  for (int i = 0; i < nf; ++i) out[i] = alego_point{kp[(size_t)i * KF_POSE_W + 0], kp[(size_t)i * KF_POSE_W + 1], kp[(size_t)i * KF_POSE_W + 2], (float)i};   // saveMapCB :833-838
  return nf;
}
// ---- the occupancy grid (alego_occ_*; kernels_occ.hip) ----
bool lm_host_occ_on(LmHost* lm) { return lm && lm->occ_on; }
int lm_host_occ_enable(LmHost* lm, const alego_occ_opts* opts, std::string* err) {
  if (const char* why = occ_opts_fault(opts)) { *err = std::string("occ_enable: ") + why; return ALEGO_ERR_ARG; }
  OccDev D = {};
  D.G = occ_grid(opts);
  const size_t cells = occ_cells(D.G);
  if (!(A(lm, &D.hits, cells, err) && A(lm, &D.passes, cells, err) && A(lm, &D.stats, ALEGO_OCC_STATS, err))) {
    lm->mem.release(D.hits); lm->mem.release(D.passes);
    return ALEGO_ERR_HIP;
  }
  lm->occ = D; lm->occ_opts = *opts; lm->occ_on = true;
  return 0;
}
int lm_host_occ_set_piece(LmHost* lm, int piece) { lm->occ_piece = piece; return 0; }
int lm_host_occ_clear(LmHost* lm, std::string* err) {
  launch_occ_clear(lm->occ, lm->st[0]);
  return DevTry("occ_clear", err, "clearing").wait(lm->st[0]);
}
// the work list of frames [first, first + n) of `slot` (n > 0) in lm->occ_items: (frame, chunk of OCC_T selected points), frames ascending; returns the
// items (0: no point is selected) or an error
static int occ_work_items(LmHost* lm, int slot, int first, int n, int kinds, const char* what, std::string* err) {
  const LmCtx& L = lm->L;
  std::vector<int> tab((size_t)n * AT_W);
  DevTry c(what, err);
  if (c.down(tab, arc_tab_of(L, slot, first))) return c;
  std::vector<int2> items;
  for (int f = 0; f < n; ++f) {
    const int sel = kf_sel_count(kf_arc_frame(L, slot, first + f, tab.data() + (size_t)f * AT_W), kinds);
    for (int c = 0; c * OCC_T < sel; ++c) items.push_back(make_int2(first + f, c));
  }
  if (c.took(lm->occ_items.reserve(items.size())).up(lm->occ_items.p, items)) return c;
  return (int)items.size();
}
int lm_host_occ_integrate(LmHost* lm, int slot, int first, int n, int kinds, int64_t* stats, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;   // (behind the slot's own stream: archive appends happen there)
  if (!(kinds & KF_SEL_ALL)) { *err = "occ_integrate: kinds must select surf / corner / outlier"; return ALEGO_ERR_ARG; }
  kinds &= KF_SEL_ALL;
  const int nf = st[AS_FRAMES];
  if (first < 0 || n < -1 || first > nf || (n >= 0 && n > nf - first)) { *err = "occ_integrate: range beyond the archived frames"; return ALEGO_ERR_ARG; }
  if (n < 0) n = nf - first;
  if (stats) for (int k = 0; k < ALEGO_OCC_STATS; ++k) stats[k] = 0;
  if (n == 0) return 0;
  const LmCtx& L = lm->L;
  const int n_items = occ_work_items(lm, slot, first, n, kinds, "occ_integrate", err);
  if (n_items <= 0) return n_items;
  hipStream_t s = stream_of_slot(lm, slot);
  if (hipMemsetAsync(lm->occ.stats, 0, ALEGO_OCC_STATS * sizeof(unsigned long long), s) != hipSuccess) { *err = "occ_integrate: upload failed"; return ALEGO_ERR_HIP; }
  launch_occ_cast(L, lm->occ, slot, kinds, lm->occ_items.p, n_items, lm->occ_piece, s);
  unsigned long long got[ALEGO_OCC_STATS];
  if (int r = DevTry("occ_integrate", err, "ray casting").wait(s).down(got, lm->occ.stats)) return r;
  if (stats) for (int k = 0; k < ALEGO_OCC_STATS; ++k) stats[k] = (int64_t)got[k];
  return 0;
}
int lm_host_occ_get(LmHost* lm, uint32_t* hits, uint32_t* passes, std::string* err) {
  const size_t cells = occ_cells(lm->occ.G);
  DevTry c("occ_get", err, "copy");
  if (hits) c.down(hits, lm->occ.hits, cells);
  if (passes) c.down(passes, lm->occ.passes, cells);
  return c;
}
int lm_host_occ_classify(LmHost* lm, const alego_occ_rule& rule, int collapse_z, int8_t* out, std::string* err) {
  const OccGrid& G = lm->occ.G;
  const size_t n_out = collapse_z ? (size_t)G.n[0] * G.n[1] : occ_cells(G);
  if (lm->occ_cls.reserve(n_out) != hipSuccess) { *err = "occ_classify: allocation failed"; return ALEGO_ERR_HIP; }
  launch_occ_classify(lm->occ, rule, collapse_z, lm->occ_cls.p, lm->st[0]);
  return DevTry("occ_classify", err, "classification").wait(lm->st[0]).down(out, lm->occ_cls.p, n_out);
}
int lm_host_occ_set(LmHost* lm, const uint32_t* hits, const uint32_t* passes, std::string* err) {
  const size_t cells = occ_cells(lm->occ.G);
  DevTry c("occ_set", err, "copy");
  if (hits) c.up(lm->occ.hits, hits, cells);
  if (passes) c.up(lm->occ.passes, passes, cells);
  return c;
}
// ---- the clearance field and the cost map (alego_occ_distance / alego_occ_costmap; kernels_edt.hip) ----
// Classifies and enqueues the transform on st[0]; *d2 is the device array that will hold the result, dom the domain.  Nothing is awaited.
static int edt_enqueue(LmHost* lm, const alego_occ_rule& rule, int collapse_z, int unknown_is_obstacle, int32_t max_cells, const char* what, int32_t* dom, double* s,
                       uint32_t** d2, std::string* err) {
  const OccGrid& G = lm->occ.G;
  const char* why = edt_domain(G.n, G.cell, collapse_z, dom, s);
  if (!why) why = edt_dims_fault(dom, max_cells);
  if (why) { *err = std::string(what) + ": " + why; return ALEGO_ERR_ARG; }
  const size_t cells = (size_t)dom[0] * dom[1] * dom[2];
  const bool env = dom[1] > 1 || dom[2] > 1;
  if (lm->occ_cls.reserve(cells) != hipSuccess || lm->edt_a.reserve(cells) != hipSuccess || lm->edt_stats.reserve(ALEGO_EDT_STATS) != hipSuccess ||
      (env && (lm->edt_b.reserve(cells) != hipSuccess || lm->edt_env.reserve(cells) != hipSuccess))) { *err = std::string(what) + ": allocation failed"; return ALEGO_ERR_HIP; }
  launch_occ_classify(lm->occ, rule, collapse_z, lm->occ_cls.p, lm->st[0]);
  EdtWork W = {lm->occ_cls.p, {dom[0], dom[1], dom[2]}, unknown_is_obstacle ? 1 : 0, (uint32_t)max_cells * (uint32_t)max_cells, lm->edt_a.p, lm->edt_b.p, lm->edt_env.p,
               env ? cells : 0, lm->edt_stats.p};
  *d2 = launch_edt(W, lm->st[0]);
  return 0;
}
static int edt_stats_out(LmHost* lm, int64_t* stats, const char* what, std::string* err) {
  unsigned long long got[ALEGO_EDT_STATS];
  if (int r = DevTry(what, err, "copy").down(got, lm->edt_stats.p)) return r;
  if (stats) { stats[ALEGO_EDT_SOURCES] = (int64_t)got[ALEGO_EDT_SOURCES]; stats[ALEGO_EDT_FAR_CELLS] = (int64_t)got[ALEGO_EDT_FAR_CELLS]; stats[ALEGO_EDT_MAX_D2] = (int64_t)got[ALEGO_EDT_MAX_D2] - 1; }
  return 0;
}
int lm_host_occ_distance(LmHost* lm, const alego_occ_rule& rule, const alego_occ_dist_opts& o, uint32_t* d2, int64_t* stats, std::string* err) {
  int32_t dom[3]; double s; uint32_t* dev = nullptr;
  if (int r = edt_enqueue(lm, rule, o.collapse_z, o.unknown_is_obstacle, o.max_cells, "occ_distance", dom, &s, &dev, err)) return r;
  DevTry c("occ_distance", err, "the transform");
  if (c.wait(lm->st[0])) return c;
  if (d2 && c.at("copy").down(d2, dev, (size_t)dom[0] * dom[1] * dom[2])) return c;
  return stats ? edt_stats_out(lm, stats, "occ_distance", err) : 0;
}
int lm_host_occ_costmap(LmHost* lm, const alego_occ_rule& rule, int collapse_z, int unknown_is_obstacle, const alego_occ_inflation& infl, uint8_t* out, std::string* err) {
  const OccGrid& G = lm->occ.G;
  int32_t dom[3], r = 0; double s;
  const char* why = edt_domain(G.n, G.cell, collapse_z, dom, &s);
  if (!why) why = edt_inflation_fault(s, &infl, &r);
  if (!why) why = edt_dims_fault(dom, r);   // (before anything is allocated; edt_enqueue asks again)
  if (why) { *err = std::string("occ_costmap: ") + why; return ALEGO_ERR_ARG; }
  std::vector<uint8_t> table((size_t)r * r + 1);
  edt_cost_table(s, &infl, r, table.data());
  const size_t cells = (size_t)dom[0] * dom[1] * dom[2];
  if (lm->edt_table.reserve(table.size()) != hipSuccess || lm->edt_cost.reserve(cells) != hipSuccess) { *err = "occ_costmap: allocation failed"; return ALEGO_ERR_HIP; }
  DevTry c("occ_costmap", err);
  if (c.up(lm->edt_table.p, table)) return c;
  uint32_t* dev = nullptr;
  if (int rc = edt_enqueue(lm, rule, collapse_z, unknown_is_obstacle, r, "occ_costmap", dom, &s, &dev, err)) return rc;
  launch_edt_cost(lm->occ_cls.p, dev, cells, unknown_is_obstacle ? 1 : 0, lm->edt_table.p, (int)table.size(), infl.inflate_unknown ? 1 : 0, lm->edt_cost.p, lm->st[0]);
  return c.at("the cost map").wait(lm->st[0]).down(out, lm->edt_cost.p, cells);
}
// ---- the static map (alego_occ_mark / alego_map_assemble_static; kernels_occ.hip) ----
// Enqueues map_offsets and occ_mark over every frame of `slot` on its stream: verdicts in lm->st_verdict, transformed points in gv.out, both in
// assembly order.  *n_sel = the selected points; `limit` >= 0 refuses (ALEGO_ERR_CAPACITY, before any launch) more selected points than that.
static int static_mark(LmHost* lm, int slot, int kinds, const alego_static_rule& rule, int limit, const char* what, OccStatic* S, int* n_sel, std::string* err) {
  int st[AS_W];
  if (int r = map_stat(lm, slot, st, err)) return r;
  const LmCtx& L = lm->L;
  const int nf = st[AS_FRAMES];
  GvCtx& G = lm->gv;
  if (int r = gv_reserve(&G, L.arc_points_cap, err)) return r == -3 ? ALEGO_ERR_CAPACITY : ALEGO_ERR_HIP;
  const int n_items = nf > 0 ? occ_work_items(lm, slot, 0, nf, kinds & KF_SEL_ALL, what, err) : 0;
  if (n_items < 0) return n_items;
  hipStream_t s = stream_of_slot(lm, slot);
  launch_map_offsets(L, slot, nf, kinds & KF_SEL_ALL, lm->arc_off, G.cnt, s);
  int n = 0;
  if (int r = DevTry(what, err, "offsets").wait(s).down(&n, G.cnt, 1)) return r;
  if (n < 0 || n > G.cap) { *err = std::string(what) + ": the archive holds more points than its capacity"; return ALEGO_ERR_HIP; }
  if (limit >= 0 && n > limit) { *err = std::string(what) + ": output capacity"; return ALEGO_ERR_CAPACITY; }
  if (lm->st_verdict.reserve(std::max(n, 1)) != hipSuccess || lm->st_kept.reserve(std::max(n_items, 1)) != hipSuccess ||
      lm->st_off.reserve((size_t)n_items + 1) != hipSuccess || lm->st_stats.reserve(ALEGO_STATIC_VERDICTS) != hipSuccess) { *err = std::string(what) + ": allocation failed"; return ALEGO_ERR_HIP; }
  *S = OccStatic{lm->occ_items.p, n_items, lm->arc_off, n, lm->st_verdict.p, G.out, lm->st_kept.p, lm->st_off.p, lm->st_stats.p};
  launch_occ_mark(L, lm->occ, *S, rule, slot, kinds & KF_SEL_ALL, s);
  *n_sel = n;
  return 0;
}
static int static_stats(LmHost* lm, int64_t* stats, const char* what, std::string* err) {
  unsigned long long got[ALEGO_STATIC_VERDICTS];
  if (int r = DevTry(what, err).down(got, lm->st_stats.p)) return r;
  if (stats) for (int k = 0; k < ALEGO_STATIC_VERDICTS; ++k) stats[k] = (int64_t)got[k];
  return 0;
}
int lm_host_occ_mark(LmHost* lm, int slot, int kinds, const alego_static_rule& rule, uint8_t* verdict, int cap, int64_t* stats, std::string* err) {
  if ((kinds & ~15) || !(kinds & KF_SEL_ALL)) { *err = "occ_mark: kinds must select surf / corner / outlier (optionally | FRAME_ID)"; return ALEGO_ERR_ARG; }
  if (cap < 0 || (cap > 0 && !verdict)) { *err = "occ_mark: a capacity without a buffer, or a negative one"; return ALEGO_ERR_ARG; }
  const bool count_only = !verdict && cap == 0;
  OccStatic S;
  int n = 0;
  if (int r = static_mark(lm, slot, kinds, rule, count_only ? -1 : cap, "occ_mark", &S, &n, err)) return r;
  DevTry c("occ_mark", err, "marking");
  if (c.wait(stream_of_slot(lm, slot))) return c;
  if (int r = static_stats(lm, stats, "occ_mark", err)) return r;
  if (!count_only && c.at("copy").down(verdict, S.verdict, (size_t)n)) return c;
  return n;
}
int lm_host_map_assemble_static(LmHost* lm, int slot, int kinds, float leaf, const alego_static_rule& rule, alego_point* out, int cap, int64_t* stats, std::string* err) {
  if ((kinds & ~15) || !(kinds & KF_SEL_ALL)) { *err = "map_assemble_static: kinds must select surf / corner / outlier (optionally | FRAME_ID)"; return ALEGO_ERR_ARG; }
  if (cap < 0) { *err = "map_assemble_static: negative capacity"; return ALEGO_ERR_ARG; }
  OccStatic S;
  int n = 0;
  if (int r = static_mark(lm, slot, kinds, rule, -1, "map_assemble_static", &S, &n, err)) return r;
  hipStream_t s = stream_of_slot(lm, slot);
  GvCtx& G = lm->gv;
  launch_occ_emit(S, kinds, G.in, G.cap, G.cnt, s);   // the kept points end where gv_filter reads its input
  if (int r = DevTry("map_assemble_static", err, "compaction").wait(s)) return r;
  if (int r = static_stats(lm, stats, "map_assemble_static", err)) return r;
  return assembled_out(lm, s, leaf, out, cap, "map_assemble_static", err);
}
int lm_host_get_local_map(LmHost* lm, int slot, alego_point* corner, int corner_cap, alego_point* surf, int surf_cap, int* n_out, std::string* err) {
  const LmCtx& L = lm->L;
  int li[LI_COUNT];
  DevTry c("get_local_map", err, "device read");
  if (c.wait(stream_of_slot(lm, slot)).down(li, L.li + (size_t)slot * LI_COUNT)) return c;
  const int nc = li[LI_KDS_C], ns = li[LI_KDS_S];
  n_out[0] = nc; n_out[1] = ns;
  if ((corner && nc > corner_cap) || (surf && ns > surf_cap)) { *err = "get_local_map: buffer too small"; return ALEGO_ERR_CAPACITY; }
  if (corner) c.down(corner, L.map_corner_ds + (size_t)slot * L.map_cap_c, (size_t)nc);
  if (surf) c.down(surf, L.map_surf_ds + (size_t)slot * L.map_cap_s, (size_t)ns);
  return c;
}
int lm_host_voxel_grid(LmHost* lm, hipStream_t s, const alego_point* pts, int n, float leaf, alego_point* out, int cap, std::string* err) {
  GvCtx& G = lm->gv;
  if (n == 0) return copy_out(G.out, 0, out, cap, "voxel_grid", err);
  if (int r = gv_reserve(&G, n, err)) return r == -3 ? ALEGO_ERR_CAPACITY : ALEGO_ERR_HIP;
  DevTry c("voxel_grid", err, "upload");
  if (c.up(G.in, pts, (size_t)n, s).up(G.cnt, &n, 1, s).wait(s)) return c;
  if (int r = gv_filter(&G, n, leaf, s, err)) return r == -3 ? ALEGO_ERR_CAPACITY : ALEGO_ERR_HIP;
  int m = 0;
  if (c.at("filter").wait(s).down(&m, G.cnt + 1, 1)) return c;
  return copy_out(G.out, m, out, cap, "voxel_grid", err);
}
int lm_host_set_gv_small_max(LmHost* lm, int v) {
  gv_destroy(&lm->gv);   // (the one-workgroup job is re-created with the new capacity by the next call)
  lm->gv.small_max = std::max(0, v);
  return 0;
}
