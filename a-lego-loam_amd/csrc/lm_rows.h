// lm_rows.h — what a registration row of LaserMapping is: the record lm_fit leaves per query (L.blocks), where a query's row lies, the record
// lm_solve streams from HBM (L.crows), the structure of arrays it keeps in LDS with the split of its budget, the two row types with their readers,
// their evaluation into the 28 normal-equation scalars, and the registration guard.  Readable by a host compiler without the HIP runtime, as
// solve_rows.h is: tests/lm_rows/lm_rows_check.cpp states the layouts with literal indices and holds every writer and reader to them.
#ifndef ALEGO_LM_ROWS_H_
#define ALEGO_LM_ROWS_H_

#include <stddef.h>
#include "solve_rows.h"

#ifndef __HIPCC__
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) double2 { double x, y; };
struct alignas(16) double4 { double x, y, z, w; };
#endif

// ---- the block record: one per query, LMB_W doubles.  a | plane normal, b, d = negative_OA_dot_norm, type = BLK_EDGE, BLK_PLANE or 0 (the query
// gave no row; the other seven doubles are then stale).  A corner query q has row q, a surf query q row surf_row0 + q (kf_cap_c in a slot's
// blocks and knn: lm_knn's LM_KNN_W neighbour indices per query lie at the same rows).
enum { LMB_A = 0, LMB_B = 3, LMB_D = 6, LMB_TYPE = 7, LMB_W = 8, LM_KNN_W = 5 };
SOLVE_FN size_t lm_row_of(int kind, int q, int surf_row0) { return kind == 0 ? (size_t)q : (size_t)surf_row0 + (size_t)q; }
SOLVE_FN size_t lm_row_of_query(int i, int nqc, int surf_row0) { return i < nqc ? (size_t)i : (size_t)surf_row0 + (size_t)(i - nqc); }   // i of the nqc corner + the surf queries
SOLVE_FN void lmb_put(double* blk, const double a[3], const double b[3], double d, int type) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { blk[LMB_A + k] = a[k]; blk[LMB_B + k] = b[k]; }
  blk[LMB_D] = d;
  blk[LMB_TYPE] = (double)type;
}
SOLVE_FN void lmb_put_none(double* blk) { blk[LMB_TYPE] = 0.0; }
SOLVE_FN void lmb_put_edge(double* blk, const double a[3], const double b[3]) { lmb_put(blk, a, b, 0.0, BLK_EDGE); }
SOLVE_FN void lmb_put_plane(double* blk, const double n[3], double d) { const double z[3] = {0, 0, 0}; lmb_put(blk, n, z, d, BLK_PLANE); }
struct LmBlock { double4 lo, hi; };   // a record in registers: two 32-byte loads
SOLVE_FN LmBlock lmb_load(const double* blk) { const double4* b = reinterpret_cast<const double4*>(blk); return LmBlock{b[0], b[1]}; }
SOLVE_FN double lmb_type(const LmBlock& B) { return B.hi.w; }

// ---- the two row types (apart, so that neither carries the other's registers) and their reader from a block and the query point
struct LmEdge { double a[3], b[3], p[3]; };    // the line's two points, the query point
struct LmPlane { double n[3], d, p[3]; };      // unit normal, negative_OA_dot_norm, the query point
SOLVE_FN LmEdge lm_edge_of(const LmBlock& B, const float4& pt) { return LmEdge{{B.lo.x, B.lo.y, B.lo.z}, {B.lo.w, B.hi.x, B.hi.y}, {pt.x, pt.y, pt.z}}; }
SOLVE_FN LmPlane lm_plane_of(const LmBlock& B, const float4& pt) { return LmPlane{{B.lo.x, B.lo.y, B.lo.z}, B.hi.z, {pt.x, pt.y, pt.z}}; }

// ---- the streamed record: LMS_W doubles = the block record + the query point as a float4 (80 B, 16-byte aligned); the accepted edges in
// query order at records [0, Rc), the accepted planes behind them
enum { LMS_PT = LMB_W, LMS_W = LMB_W + 2 };
SOLVE_FN size_t lms_edge_at(int i) { return (size_t)i; }
SOLVE_FN size_t lms_plane_at(int Rc, int j) { return (size_t)Rc + (size_t)j; }
SOLVE_FN double2 lmr_d2(double x, double y) { double2 r; r.x = x; r.y = y; return r; }
SOLVE_FN void lms_put(double* rec, const LmBlock& B, const float4& pt) {
  double2* o = reinterpret_cast<double2*>(rec);
  o[0] = lmr_d2(B.lo.x, B.lo.y); o[1] = lmr_d2(B.lo.z, B.lo.w); o[2] = lmr_d2(B.hi.x, B.hi.y); o[3] = lmr_d2(B.hi.z, B.hi.w);
  *reinterpret_cast<float4*>(rec + LMS_PT) = pt;
}
SOLVE_FN LmEdge lms_edge(const double* rec) {
  const double2* b = reinterpret_cast<const double2*>(rec);
  const double2 q0 = b[0], q1 = b[1], q2 = b[2];
  const float4 pc = *reinterpret_cast<const float4*>(rec + LMS_PT);
  return LmEdge{{q0.x, q0.y, q1.x}, {q1.y, q2.x, q2.y}, {pc.x, pc.y, pc.z}};
}
SOLVE_FN LmPlane lms_plane(const double* rec) {
  const double2* b = reinterpret_cast<const double2*>(rec);
  const double2 q0 = b[0], q1 = b[1], q3 = b[3];
  const float4 pc = *reinterpret_cast<const float4*>(rec + LMS_PT);
  return LmPlane{{q0.x, q0.y, q1.x}, q3.x, {pc.x, pc.y, pc.z}};
}

// ---- the accepted rows of one registration: Rc edges and Rs planes, the first Ce / Cp of them resident in a byte budget of LDS as a structure of
// arrays — ea[k * Ce + i], eb[k * Ce + i], ep[k * Ce + i] (k < 3); pn[k * Cp + j] (k < 4: normal, d), pp[k * Cp + j] (k < 3), the f64 arrays
// first — and the others as streamed records in crows
enum { LML_EDGE_BYTES = (3 + 3) * 8 + 3 * 4, LML_PLANE_BYTES = 4 * 8 + 3 * 4 };   // ea, eb, ep | pn, pp
static_assert(LML_EDGE_BYTES == 60 && LML_PLANE_BYTES == 44, "bytes per resident edge / plane");
struct LmRows {
  int Rc, Rs, Ce, Cp;
  double *ea, *eb, *pn;
  float *ep, *pp;
  double* crows;
};
SOLVE_FN void lml_split(int Rc, int Rs, size_t budget, int* Ce, int* Cp) {   // edges first: as many as fit, then planes into what is left
  const size_t ce = budget / LML_EDGE_BYTES < (size_t)Rc ? budget / LML_EDGE_BYTES : (size_t)Rc;
  const size_t left = (budget - (size_t)LML_EDGE_BYTES * ce) / LML_PLANE_BYTES;
  *Ce = (int)ce;
  *Cp = (int)(left < (size_t)Rs ? left : (size_t)Rs);
}
struct LmLdsOff { size_t ea, eb, pn, ep, pp, end; };   // bytes from the start of the budget
SOLVE_FN LmLdsOff lml_offsets(int Ce, int Cp) {
  LmLdsOff o;
  o.ea = 0; o.eb = o.ea + (size_t)3 * 8 * Ce; o.pn = o.eb + (size_t)3 * 8 * Ce;
  o.ep = o.pn + (size_t)4 * 8 * Cp; o.pp = o.ep + (size_t)3 * 4 * Ce; o.end = o.pp + (size_t)3 * 4 * Cp;
  return o;
}
SOLVE_FN LmRows lml_make(int Rc, int Rs, unsigned char* lds, size_t budget, double* crows) {
  LmRows W;
  W.Rc = Rc; W.Rs = Rs; W.crows = crows;
  lml_split(Rc, Rs, budget, &W.Ce, &W.Cp);
  const LmLdsOff o = lml_offsets(W.Ce, W.Cp);
  W.ea = reinterpret_cast<double*>(lds + o.ea); W.eb = reinterpret_cast<double*>(lds + o.eb); W.pn = reinterpret_cast<double*>(lds + o.pn);
  W.ep = reinterpret_cast<float*>(lds + o.ep); W.pp = reinterpret_cast<float*>(lds + o.pp);
  return W;
}
SOLVE_FN void lml_put_edge(const LmRows& W, int r, const LmBlock& B, const float4& pt) {
  W.ea[r] = B.lo.x; W.ea[W.Ce + r] = B.lo.y; W.ea[2 * W.Ce + r] = B.lo.z;
  W.eb[r] = B.lo.w; W.eb[W.Ce + r] = B.hi.x; W.eb[2 * W.Ce + r] = B.hi.y;
  W.ep[r] = pt.x; W.ep[W.Ce + r] = pt.y; W.ep[2 * W.Ce + r] = pt.z;
}
SOLVE_FN void lml_put_plane(const LmRows& W, int r, const LmBlock& B, const float4& pt) {
  W.pn[r] = B.lo.x; W.pn[W.Cp + r] = B.lo.y; W.pn[2 * W.Cp + r] = B.lo.z; W.pn[3 * W.Cp + r] = B.hi.z;
  W.pp[r] = pt.x; W.pp[W.Cp + r] = pt.y; W.pp[2 * W.Cp + r] = pt.z;
}
SOLVE_FN LmEdge lml_edge(const LmRows& W, int i) {
  LmEdge e;
#pragma unroll
  for (int k = 0; k < 3; ++k) { e.a[k] = W.ea[k * W.Ce + i]; e.b[k] = W.eb[k * W.Ce + i]; e.p[k] = (double)W.ep[k * W.Ce + i]; }
  return e;
}
SOLVE_FN LmPlane lml_plane(const LmRows& W, int j) {
  LmPlane p;
#pragma unroll
  for (int k = 0; k < 3; ++k) { p.n[k] = W.pn[k * W.Cp + j]; p.p[k] = (double)W.pp[k * W.Cp + j]; }
  p.d = W.pn[3 * W.Cp + j];
  return p;
}

// ---- evaluation: EdgeCostFunction (utility.h:242-297) / PlaneCostFunction (utility.h:299-349) of one row at the pose of T, into the 28
// normal-equation scalars (FULL) or its cost alone into acc[27].  (Neither has a third point, a plane no second one: zeros, never read.)
template <int TYPE, bool FULL>
SOLVE_FN void lm_eval_row(const double p[3], const double a[3], const double b[3], double d, const PoseTerms& T, double huber, double acc[28]) {
  const double c3[3] = {0, 0, 0};
  if constexpr (FULL) {
    double res, J[6];
    eval_block(TYPE, p, a, b, c3, d, T, &res, J);
    accumulate_block(res, J, huber, acc);
  } else accumulate_cost(eval_block_residual<TYPE>(p, a, b, c3, d, T), huber, acc[27]);
}
template <bool FULL>
SOLVE_FN void lm_eval_edge(const LmEdge& e, const PoseTerms& T, double huber, double acc[28]) { lm_eval_row<BLK_EDGE, FULL>(e.p, e.a, e.b, 0.0, T, huber, acc); }
template <bool FULL>
SOLVE_FN void lm_eval_plane(const LmPlane& p, const PoseTerms& T, double huber, double acc[28]) {
  const double b3[3] = {0, 0, 0};
  lm_eval_row<BLK_PLANE, FULL>(p.p, p.n, b3, p.d, T, huber, acc);
}

// ---- the registration guard (laserMapping.cpp:350): too few corner / surf points in the scan, too small a corner map, or no map yet
// (lm_reg_skipped, lm_ctx.h: lm_knn, lm_fit and both solver paths skip the registration by this one predicate)
SOLVE_FN bool lm_guard_fails(int ncur_c, int ntotal, int kds_c, bool no_map, int min_corner, int min_surf, int min_map_corner) {
  return ncur_c < min_corner || ntotal < min_surf || kds_c < min_map_corner || no_map;
}

#endif
