// reloc.h — host interface of relocalisation in the frozen map (kernels_reloc.hip; alego_reloc_* / alego_loc_relocalize) and of the
// appearance search of a SLAM handle over its own archive, which runs the same search kernels
#ifndef ALEGO_RELOC_H_
#define ALEGO_RELOC_H_
#include "loop_ctx.h"   // LcCtx, LmCtx

struct RlCtx;   // map / query descriptors (reloc_enable); search scratch allocated by the first search and kept
int reloc_enable(RlCtx** pr, const LmCtx& L, int n_slots, double max_range, double z_offset, hipStream_t st, std::string* err);
bool reloc_enabled(const RlCtx* R);
// the map store was rebuilt (alego_loc_update_from_map): its descriptors and ring keys again, for the L.loc_n frames it holds now; nothing when relocalisation is off
int reloc_refresh(RlCtx* R, const LmCtx& L, hipStream_t st, std::string* err);
int reloc_run(RlCtx* R, LcCtx** lc, const LmCtx& L, const alego_params& P, const int* slots, int n, int n_cand, int verify, int apply, alego_reloc_result* out,
              hipStream_t st, std::string* err);
int reloc_debug_search(RlCtx** pr, const uint8_t* map_desc, int n_map, const uint8_t* q_desc, int n_q, int n_cand, int32_t* ids, int32_t* dists, int32_t* shifts,
                       hipStream_t st, std::string* err);
int reloc_debug_get(RlCtx* R, int slot, const char* name, const void** src, size_t* bytes);
// the appearance search of a SLAM handle over its own archive (alego_loop_appearance_enable / alego_loop_search_appearance); o: defaults resolved
int loop_app_enable(RlCtx** pr, const LmCtx& L, int n_slots, double max_range, double z_offset, std::string* err);
bool loop_app_enabled(const RlCtx* R);
int loop_app_run(RlCtx* R, LcCtx** lc, const LmCtx& L, const alego_params& P, const int* slots, int n, const alego_loop_app_opts& o, alego_loop_result* out,
                 alego_loop_app_info* info, hipStream_t st, std::string* err);
int loop_app_debug_get(RlCtx* R, int slot, const char* name, const void** src, size_t* bytes);   // "la_desc", "la_key"
// the slot's archive changed from frame `first` on (alego_map_thin): its descriptors stay valid below it, the rest is described again lazily
void loop_app_forget(RlCtx* R, int slot, int first);
// alego_map_align: one slot's archive aligned to another's by appearance (needs loop_app_enable); o: n_queries and n_cand resolved
int map_align_run(RlCtx* R, LcCtx** lc, const LmCtx& L, const alego_params& P, const int* src, const int* dst, int n, const alego_map_align_opts& o, alego_map_align_result* out,
                  alego_map_align_hyp* hyp, hipStream_t st, std::string* err);
void reloc_debug_stats(const RlCtx* R, int out[2]);
void reloc_ctx_set(RlCtx** pr, int what, long long v);   // what 0: pairs per chunk of the search, 1: brute force
void reloc_ctx_destroy(RlCtx* R);
#endif
