// loop_ctx.h — one ICP attempt per listed slot as kernels_loop.hip runs it (VoxelGrid(lc_leaf) of the raw sub-map, lc_grid, lc_icp), for the
// callers that bring their own source and sub-map: alego_loop_search and the appearance search gather them from the archive
// (loop_archive_gather), alego_loc_relocalize (kernels_reloc.hip) from the current scan and the frozen map store.  What an attempt is made
// of has one definition here, whoever plans it: the window (lc_window, reloc_math.h), the sizes, where a frame lands in the raw sub-map,
// the verification rounds and the alego_loop_result of a verdict.
#ifndef ALEGO_LOOP_CTX_H_
#define ALEGO_LOOP_CTX_H_
#include <hip/hip_runtime.h>

#include <functional>
#include <string>

#include "../../include/alego_mi355x.h"
#include "kf_store.h"
#include "reloc_math.h"

struct LcDet {        // lc_detect's verdict on one listed slot
  int status;         // 0 no candidate, 1 attempt, -1 the archive dropped frames
  int latest, closest, jlo, jhi;   // history frames jlo .. jhi (jhi < jlo: none)
  int n_src, n_raw;
  int src1;           // 0: the source is frame `latest` of the attempt's own slot; s + 1: of slot s (alego_map_align: another slot's archive)
  float pose_latest[6], pose_closest[6];
};
DEV_INLINE int lc_src_slot(const LcDet& D, int slot) { return D.src1 > 0 ? D.src1 - 1 : slot; }
struct LcJob { int li, slot, src_off, raw_off, cell_off, cell_cap; };   // one attempted slot of a chunk and its scratch regions
struct LcOut { int converged, iterations, n_source, n_target; double fitness; float correction[16]; };   // lc_icp's verdict on one attempt

// n_src = the points of archived frame `src` of the source's slot (lc_src_slot), n_raw = those of the window D->jlo .. D->jhi of `slot`, from the archive's tables
DEV_INLINE void lc_det_sizes(const LmCtx& L, int slot, int src, LcDet* D) {
  D->n_src = arc_tab_points(arc_tab_of(L, lc_src_slot(*D, slot), src));
  long long n = 0;
  for (int j = D->jlo; j <= D->jhi; ++j) n += arc_tab_points(arc_tab_of(L, slot, j));
  D->n_raw = (int)n;
}
// where frame f of the window starts in the job's raw sub-map: behind frames jlo .. f - 1, points(j) = the points the gather writes for frame j
template <class F> DEV_INLINE float4* lc_frame_out(float4* raw, const LcJob& J, const LcDet& D, int f, F points) {
  int off = 0;
  for (int j = D.jlo; j < f; ++j) off += points(j);
  return raw + J.raw_off + off;
}

struct LcCtx;   // the batched loop-closure search: detection / chunk scratch, allocated by the first call and kept with the handle
void loop_ctx_destroy(LcCtx* C);
void loop_ctx_set_budget(LcCtx** pc, long long points);
int loop_search(LcCtx** pc, const LmCtx& L, const alego_params& P, int n_slots, const int* slots, int n, alego_loop_result* res, hipStream_t st, std::string* err);
int loop_debug_nn1(const alego_point* tgt, int n_tgt, const alego_point* q, int nq, int32_t* idx, float* d2, hipStream_t st, std::string* err);
// kernels_icp.hip: one attempt with the frames the host brings (alego_loop_closure_icp)
int icp_run(const alego_params& P, const alego_kf_in* latest, const alego_kf_in* history, int n_history, alego_icp_result* out,
            alego_point* target_out, int target_cap, hipStream_t st, std::string* err);
// fills src + jobs[j].src_off (det[jobs[j].li].n_src points) and raw + jobs[j].raw_off (n_raw points) of the J jobs of a chunk on `st`; nfr = 2 + 2 lc_search_num
typedef std::function<void(const LcJob* jobs, const LcDet* det, int J, int nfr, float4* src, float4* raw, hipStream_t st)> LcGather;
// det[0 .. n) on the host (any n: entries run in pieces of the context's list capacity, which is at least n_slots, and may repeat a slot; status == 1: attempted, with n_src, n_raw and whatever the gather reads filled in) -> out[i] of every attempt.
// Chunked under the context's point budget (ALEGO_LC_BUDGET): chunking never changes a result.  Synchronous on `st`.
int loop_attempts(LcCtx** pc, const alego_params& P, int n_slots, const int* slots, const LcDet* det, int n, const LcGather& gather, LcOut* out, hipStream_t st, std::string* err);
// the gather of attempts read from the archive (lc_gather): source = frame det.latest of the source's slot (lc_src_slot) under det.pose_latest,
// sub-map = frames jlo .. jhi of the job's slot under their archived poses
LcGather loop_archive_gather(const LmCtx& L);
// Verification rounds over n entries: round v < rounds tries candidate v of every entry that has one and is not accepted yet; the
// first acceptance ends the entry, and a round with nothing left to try ends the rounds.  plan(i, v, D): fill attempt (i, v) into the zeroed *D as
// loop_attempts takes it and return true, or decline; verdict(i, v, D, O): the verdict O on attempt D of (i, v) -> was it accepted?
typedef std::function<bool(int i, int v, LcDet* D)> LcPlan;
typedef std::function<bool(int i, int v, const LcDet& D, const LcOut& O)> LcVerdict;
int loop_rounds(LcCtx** pc, const alego_params& P, int n_slots, const int* slots, int n, int rounds, const LcGather& gather, const LcPlan& plan, const LcVerdict& verdict, hipStream_t st,
                std::string* err);
// r <- the verdict O on attempt D: closest_id, the ICP's numbers, t_correct / between (alego_loop_constraint), noise_variance, status 2 when
// converged && fitness <= fitness_max (:697) and 1 otherwise; returns whether it was accepted
bool loop_result_fill(const LcDet& D, const LcOut& O, double fitness_max, alego_loop_result* r);
#endif
