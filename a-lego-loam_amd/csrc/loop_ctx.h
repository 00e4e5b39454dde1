// loop_ctx.h — one ICP attempt per listed slot as kernels_loop.hip runs it (VoxelGrid(lc_leaf) of the raw sub-map, lc_grid, lc_icp), for the
// callers that bring their own source and sub-map: alego_loop_search gathers them from the archive, alego_loc_relocalize (kernels_reloc.hip)
// from the current scan and the frozen map store.
#ifndef ALEGO_LOOP_CTX_H_
#define ALEGO_LOOP_CTX_H_
#include <hip/hip_runtime.h>

#include <functional>
#include <string>

#include "../../include/alego_mi355x.h"

struct LcDet {        // lc_detect's verdict on one listed slot
  int status;         // 0 no candidate, 1 attempt, -1 the archive dropped frames
  int latest, closest, jlo, jhi;   // history frames jlo .. jhi (jhi < jlo: none)
  int n_src, n_raw, pad;
  float pose_latest[6], pose_closest[6];
};
struct LcJob { int li, slot, src_off, raw_off, cell_off, cell_cap; };   // one attempted slot of a chunk and its scratch regions
struct LcOut { int converged, iterations, n_source, n_target; double fitness; float correction[16]; };   // lc_icp's verdict on one attempt

struct LmCtx;
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
// det[0 .. n) on the host (n <= n_slots; status == 1: attempted, with n_src, n_raw and whatever the gather reads filled in) -> out[i] of every attempt.
// Chunked under the context's point budget (ALEGO_LC_BUDGET): chunking never changes a result.  Synchronous on `st`.
int loop_attempts(LcCtx** pc, const alego_params& P, int n_slots, const int* slots, const LcDet* det, int n, const LcGather& gather, LcOut* out, hipStream_t st, std::string* err);
#endif
