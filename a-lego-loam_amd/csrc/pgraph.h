// pgraph.h — host interface of the key-pose graph (kernels_graph.hip)
#ifndef ALEGO_PGRAPH_H_
#define ALEGO_PGRAPH_H_
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/alego_mi355x.h"

struct LmCtx;
struct PgCtx;   // chunk scratch, the staging buffer of appended loop edges and the applied-slot flags: allocated on first use, kept with the handle

// one loop edge on its way to the device: written at `index` of `slot`; the last entry of a slot leaves its correction and the loop count
struct PgAppend { int slot, index, last, pad; alego_graph_edge e; float corr[16]; };

void graph_ctx_destroy(PgCtx* C);
void graph_ctx_set_budget(PgCtx** pc, long long bytes);
// out = {chain edges (= archived frames), loop edges, loop_closed_, poses of the last estimate}
int graph_status(const LmCtx& L, int slot, int* out4, std::string* err);
int graph_get_edges(const LmCtx& L, int slot, int kind, int first, int n, alego_graph_edge* out, std::string* err);
int graph_set_edges(const LmCtx& L, int slot, int first, int n, const alego_graph_edge* chain, std::string* err);
int graph_append(PgCtx** pc, const LmCtx& L, int n_slots, const std::vector<PgAppend>& in, hipStream_t st, std::string* err);
int graph_get_estimate(const LmCtx& L, int slot, int first, int n, double* poses12, std::string* err);
int graph_optimize(PgCtx** pc, const LmCtx& L, int n_slots, const int* slots, int n, const alego_graph_opts& opt, alego_graph_result* out,
                   std::vector<int>* apply_out, hipStream_t st, std::string* err);
int graph_upload_apply(PgCtx* C, const std::vector<int>& apply, const int** dev, hipStream_t st, std::string* err);
// correctPoses on the device for the slots flagged in apply_dev (lm_host_graph_apply)
void launch_pg_apply(const LmCtx& L, const int* apply_dev, int n_slots, hipStream_t st);
void launch_pg_retransform(const LmCtx& L, const int* apply_dev, int slot0, int n, int j, hipStream_t st);
void launch_pg_sorted(const LmCtx& L, const int* apply_dev, int slot0, int n, int all, hipStream_t st);
int graph_residuals_host(const double* poses12, int n_poses, const alego_graph_edge* edges, int n_edges, double* whitened6, double* jac_from36, double* jac_to36);
// marginal covariances and the consistency of candidate edges (kernels_pgcov.hip).  graph_check: active[i] == 0 (active
// may be null) leaves candidate i unjudged with status 0
int graph_marginals(PgCtx** pc, const LmCtx& L, int n_slots, const int* slots, int n, int cap, double* cov36, alego_graph_cov_result* out, hipStream_t st,
                    std::string* err);
int graph_check(PgCtx** pc, const LmCtx& L, int n_slots, const int* slots, int n, const alego_graph_edge* e, const char* active, alego_graph_check* out,
                hipStream_t st, std::string* err);
int graph_covariance_host(const double* poses12, int n_poses, const alego_graph_edge* edges, int n_edges, const int* pairs, int n_pairs, double* marg36, double* pair36);
int graph_check_host(const double* poses12, int n_poses, const alego_graph_edge* edges, int n_edges, const alego_graph_edge* cand, int n_cand, alego_graph_check* out);
#endif
