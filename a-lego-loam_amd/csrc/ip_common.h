// ip_common.h — device pieces shared by the ImageProjection kernels (kernels_ip.hip: the multi-kernel path; kernels_ipf.hip: the
// one-workgroup-per-stream fused path; kernels_ipb.hip: the banded path): the cell of an input point, the ground test, the segmentation's
// edge predicate, the records and the count scan of the ordered compaction (their rules: ip_rules.h) and the 16-bit LDS union-find.
#ifndef ALEGO_IP_COMMON_H_
#define ALEGO_IP_COMMON_H_
#include "dev_common.h"
#include "ip_rules.h"

// The cell of one input point (imageProjection.cpp:76-97; IP.cpp:91,142-172): row * H + col, or -1 when the point is rejected (row /
// column out of range, non-finite, near filter).  *valid_out = the point survives pcl::removeNaNFromPointCloud / removeClosedPointCloud,
// i.e. it counts as first / last point of the scan for the orientation block (:62-63).  Shared by ip_project and ip_fused.
DEV_INLINE int ip_point_cell(const DevCtx& d, const float4 p, bool* valid_out) {
  const alego_params& P = d.P;
  bool valid;
  int cell = -1;
    // pcl::removeNaNFromPointCloud only filters when the message is not dense (alego_params.input_is_dense); an unfiltered
    // non-finite point still counts as first / last point of the scan and is rejected by the row test (int(NaN) < 0)
    const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    valid = finite || P.input_is_dense != 0;
    if (valid && P.near_filter) {
      const float th = (float)P.near_thres;
      if (p.x * p.x + p.y * p.y + p.z * p.z < th * th) valid = false;  // IP.cpp:91
    }
    if (valid && finite) {
      // ---- fast path: cell from the boundary tables.  The reference rounds atan2f / hypotf to f32 before it divides by the
      // angular resolution, so its row / column is the cell of the TRUE angle unless that angle lies within ~7e-5 cells of a
      // boundary.  A polynomial estimate (good to 0.03 cells) picks a boundary, the exact offset to it comes from one
      // cross / dot product against the boundary's (cos, sin) (fp64 products, f32 quotient: error < 1e-6 cells), and a point
      // closer than 2.5e-4 columns / 1e-4 rows to any boundary takes the reference expressions below.  Every comparison is
      // written so that a NaN or an out-of-range estimate also lands there.
      int row = -1, col = -1;
      bool slow = true;
      {
        const float h2 = p.x * p.x + p.y * p.y, hf = __builtin_amdgcn_sqrtf(h2);   // (v_sqrt_f32 / v_rcp_f32: 1 ulp is plenty here)
        bool okr = (d.ip_fast & 1) && hf > 1e-3f && hf < 1e6f && fabsf(p.z) < 1e6f;
        const float t = p.z * __builtin_amdgcn_rcpf(hf), t2 = t * t;
        okr = okr && fabsf(t) < 0.6f;
        const float a = t * (0.99997726f + t2 * (-0.33262347f + t2 * (0.19354346f + t2 * (-0.11643287f + t2 * (0.05265332f + t2 * -0.01172120f)))));
        const float r0 = (a * 57.29577951f + (float)P.ang_bottom) * (float)d.inv_res_y + 0.5f;
        const float kf = floorf(r0);
        okr = okr && kf >= -3.0f && kf <= (float)(d.NS + 1);
        const int kk = okr ? (int)kf : 0;
        const double2 cs = d.ip_rowtab[kk + 3];
        const float cr = (float)((double)p.z * cs.x - (double)hf * cs.y), dt = (float)((double)hf * cs.x + (double)p.z * cs.y);
        const float q = cr * __builtin_amdgcn_rcpf(dt);
        const float frac = q * (1.0f - q * q * 0.33333333f) * (57.29577951f * (float)d.inv_res_y);
        const float fl = floorf(frac), dlo = frac - fl, dhi = 1.0f - dlo;
        const int rfl = kk + (int)fl;   // floor of the reference's r; (int)r truncates: r in (-1, 1) is row 0, so 0 is no boundary
        okr = okr && dt > 0.0f && frac > -1.0f && frac < 2.0f && (dlo >= 1e-4f || rfl == 0) && (dhi >= 1e-4f || rfl + 1 == 0);
        // columns
        const float ax = fabsf(p.x), ay = fabsf(p.y), mn = fminf(ax, ay), mx = fmaxf(ax, ay);
        bool okc = (d.ip_fast & 2) && mx > 1e-3f && mx < 1e6f;
        const float u = mn * __builtin_amdgcn_rcpf(mx), u2 = u * u;
        float b = u * (0.99997726f + u2 * (-0.33262347f + u2 * (0.19354346f + u2 * (-0.11643287f + u2 * (0.05265332f + u2 * -0.01172120f)))));
        b = ay > ax ? 1.57079633f - b : b;
        b = p.x < 0.0f ? 3.14159265f - b : b;
        b = p.y < 0.0f ? -b : b;
        const float cf = floorf((6.28318531f - b) * (57.29577951f * (float)d.inv_res_x)) - (float)d.ip_cmin;
        okc = okc && cf >= 0.0f && cf <= (float)(d.ip_ncb - 1);
        const int ci = okc ? (int)cf : 0;
        const double2 cc = d.ip_coltab[ci];
        const float crc = (float)(-(double)p.y * cc.x - (double)p.x * cc.y), dtc = (float)((double)p.x * cc.x - (double)p.y * cc.y);
        const float qc = crc * __builtin_amdgcn_rcpf(dtc);
        const float fc = qc * (1.0f - qc * qc * 0.33333333f) * (57.29577951f * (float)d.inv_res_x);
        const float flc = floorf(fc), dloc = fc - flc;
        okc = okc && dtc > 0.0f && fc > -1.0f && fc < 2.0f && dloc >= 2.5e-4f && 1.0f - dloc >= 2.5e-4f;
        if (okr && okc) {
          slow = false;
          row = rfl >= 0 ? rfl : (rfl == -1 ? 0 : -1);
          col = d.ip_cmin + ci + (int)flc;
          if (col >= d.H) col -= d.H;
        }
      }
      if (slow) {
      // imageProjection.cpp:79-80 (IP.cpp:142-172 for the RFANS table)
      // (a * 180.0) / M_PI and x / ang_res are IEEE fp64 divisions in the reference (~35 instructions each here).  The
      // integer part of the result only depends on the exact quotient when it lies within rounding error of an
      // integer: multiply by the reciprocals first and redo the reference expression only in that case.
      const double va = (double)d_atan2f(p.z, d_hypotf(p.x, p.y)) * 180.0;
      if (P.laser_type == ALEGO_LASER_UNIFORM) {
        const double r = (va * (1.0 / M_PI) + P.ang_bottom) * d.inv_res_y + 0.5;
        row = (int)r;
        if (fabs(r - rint(r)) < 1e-9 * (1.0 + fabs(r))) row = (int)((va / M_PI + P.ang_bottom) / P.ang_res_y + 0.5);
      } else {  // RFANS ring table (IP.cpp:142-172)
        const double vertical_ang = va / M_PI;
        if (vertical_ang > 4.5) row = (int)(13 + (vertical_ang - 5.) / 3 + 0.5);
        else if (vertical_ang > 0.5) row = (int)(11 + (vertical_ang - 1.0) / 2 + 0.5);
        else if (vertical_ang > -7.) row = (int)(10.5 + vertical_ang);
        else if (vertical_ang > -8.5) row = 3;
        else if (vertical_ang > -10.5) row = 2;
        else if (vertical_ang > -13.5) row = 1;
        else row = 0;
      }
      // :87-97
      const double ha = ((double)(-d_atan2f(p.y, p.x)) + 2 * M_PI) * 180.0;
      const double cfast = ha * (1.0 / M_PI) * d.inv_res_x;
      col = (int)cfast;
      if (fabs(cfast - rint(cfast)) < 1e-9 * (1.0 + fabs(cfast))) col = (int)((ha / M_PI) / P.ang_res_x);
      if (col >= d.H) col -= d.H;
      }
      if (row >= 0 && row < d.NS && col >= 0 && col < d.H) cell = col + row * d.H;
    }
  *valid_out = valid;
  return cell;
}

// Quick decision for ip_fused's first pass.  The row / column of a point is the cell of its TRUE elevation / azimuth unless that angle lies
// within the reference's own rounding (~3e-5 cells) of a cell boundary, so a cheap estimate of both angles whose error is bounded decides every
// point that is not NEAR a boundary; the others (a few per cent of a real scan) are deferred to ip_point_cell (table refinement or the
// reference expressions).  Error budget of the estimate: the odd degree-11 polynomial for atan on [0, 1] is within 1.8e-6 rad of atan in f32
// (tests/test_oracle.py::test_quick_projection_polynomial_bound evaluates it on 2M arguments), v_rcp / v_sqrt (1 ulp) and the quadrant fix-ups
// add < 1.5e-6 rad, the product with 180 / (pi res) two roundings of a value <= 1.5 H: 4e-6 rad and 4e-7 H cells in total are charged, twice
// over, in the margins below (at least 0.02 columns / 0.005 rows).  Nothing here has to be bit-exact, so FMA contraction is allowed.
// Returns true when decided: *cell_out = row * H + col, or -1 when the point has no cell (filtered, non-finite, outside the image).
// the uniform values of ip_point_quick, converted once (round 5: read from the kernel argument inside ip_fused_t's point loop they were 18 scalar loads and
// 8 v_cvt_f32_f64 per iteration of four points)
struct IpQuickConst {
  float th2;          // near_thres^2 as the reference squares it (f32), < 0: no near filter
  float ang_bottom, inv_res_y, col_scale;   // (float)P.ang_bottom, (float)(1 / ang_res_y), 57.29577951f * (float)(1 / ang_res_x)
  float two_h;        // (float)(2 H)
  int H, NS, dense, fast;
};
DEV_INLINE IpQuickConst ip_quick_const(const DevCtx& d) {
  IpQuickConst c;
  const float th = (float)d.P.near_thres;
  c.th2 = d.P.near_filter ? th * th : -1.0f;
  c.ang_bottom = (float)d.P.ang_bottom; c.inv_res_y = (float)d.inv_res_y; c.col_scale = 57.29577951f * (float)d.inv_res_x;
  c.two_h = (float)(2 * d.H);
  c.H = d.H; c.NS = d.NS; c.dense = d.P.input_is_dense != 0; c.fast = (d.ip_fast & 3) == 3;
  return c;
}
DEV_INLINE bool ip_point_quick(const IpQuickConst& c, const float4 p, float mr, float mc, bool* valid_out, int* cell_out) {
  const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  bool valid = finite || c.dense;
  if (valid && p.x * p.x + p.y * p.y + p.z * p.z < c.th2) valid = false;  // IP.cpp:91 (same expression as ip_point_cell; th2 < 0: filter off, NaN compares false)
  *valid_out = valid;
  *cell_out = -1;
  if (!(valid && finite)) return true;
  if (!c.fast) return false;
  bool ok;
  int rfl, col;
  {
#pragma clang fp contract(fast)
    const float h2 = p.x * p.x + p.y * p.y, hf = __builtin_amdgcn_sqrtf(h2);
    const float t = p.z * __builtin_amdgcn_rcpf(hf), t2 = t * t;
    ok = hf > 1e-3f && hf < 1e6f && fabsf(t) < 0.6f;
    const float a = t * (0.99997726f + t2 * (-0.33262347f + t2 * (0.19354346f + t2 * (-0.11643287f + t2 * (0.05265332f + t2 * -0.01172120f)))));
    const float r0 = (a * 57.29577951f + c.ang_bottom) * c.inv_res_y + 0.5f;
    const float rf = floorf(r0), fr = r0 - rf;
    ok = ok && fr >= mr && fr <= 1.0f - mr && rf >= -64.0f && rf <= 4096.0f;
    rfl = (int)rf;
    const float ax = fabsf(p.x), ay = fabsf(p.y), mn = fminf(ax, ay), mx = fmaxf(ax, ay);
    ok = ok && mx > 1e-3f && mx < 1e6f;
    const float u = mn * __builtin_amdgcn_rcpf(mx), u2 = u * u;
    float b = u * (0.99997726f + u2 * (-0.33262347f + u2 * (0.19354346f + u2 * (-0.11643287f + u2 * (0.05265332f + u2 * -0.01172120f)))));
    b = ay > ax ? 1.57079633f - b : b;
    b = p.x < 0.0f ? 3.14159265f - b : b;
    b = p.y < 0.0f ? -b : b;
    const float c0 = (6.28318531f - b) * c.col_scale;   // (-atan2f(y, x) + 2 pi) * 180 / pi / ang_res_x (:87-95)
    const float cf = floorf(c0), fc = c0 - cf;
    ok = ok && fc >= mc && fc <= 1.0f - mc && cf >= 0.0f && cf < c.two_h;
    col = (int)cf;
  }
  if (!ok) return false;   // (a NaN anywhere fails a comparison above)
  const int row = rfl >= 0 ? rfl : (rfl == -1 ? 0 : -1);   // (int)r truncates: r in (-1, 1) is row 0
  if (col >= c.H) col -= c.H;
  if (row >= 0 && row < c.NS && col >= 0 && col < c.H) *cell_out = col + row * c.H;
  return true;
}
DEV_INLINE bool ip_point_quick(const DevCtx& d, const float4 p, float mr, float mc, bool* valid_out, int* cell_out) {
  return ip_point_quick(ip_quick_const(d), p, mr, mc, valid_out, cell_out);
}
// the same decision without a branch (ip_fused_t's point loop evaluates four points per iteration: the early returns above were four nests of exec-mask
// bookkeeping): every expression is evaluated for every point — a non-finite or filtered point only produces values nobody looks at — and the three
// outcomes are selected at the end.  Returns "decided"; *cell_out as above.
DEV_INLINE bool ip_point_quick_bf(const IpQuickConst& c, const float4 p, float mr, float mc, bool* valid_out, int* cell_out) {
  const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  const bool valid = (finite || c.dense) && !(p.x * p.x + p.y * p.y + p.z * p.z < c.th2);
  bool ok;
  int rfl, col;
  {
#pragma clang fp contract(fast)
    const float h2 = p.x * p.x + p.y * p.y, hf = __builtin_amdgcn_sqrtf(h2);
    const float t = p.z * __builtin_amdgcn_rcpf(hf), t2 = t * t;
    ok = hf > 1e-3f && hf < 1e6f && fabsf(t) < 0.6f;
    const float a = t * (0.99997726f + t2 * (-0.33262347f + t2 * (0.19354346f + t2 * (-0.11643287f + t2 * (0.05265332f + t2 * -0.01172120f)))));
    const float r0 = (a * 57.29577951f + c.ang_bottom) * c.inv_res_y + 0.5f;
    const float rf = floorf(r0), fr = r0 - rf;
    ok = ok && fr >= mr && fr <= 1.0f - mr && rf >= -64.0f && rf <= 4096.0f;
    rfl = (int)(ok ? rf : 0.0f);   // (a float -> int conversion of NaN / inf / out-of-range values is undefined: convert only what the checks above admitted)
    const float ax = fabsf(p.x), ay = fabsf(p.y), mn = fminf(ax, ay), mx = fmaxf(ax, ay);
    ok = ok && mx > 1e-3f && mx < 1e6f;
    const float u = mn * __builtin_amdgcn_rcpf(mx), u2 = u * u;
    float b = u * (0.99997726f + u2 * (-0.33262347f + u2 * (0.19354346f + u2 * (-0.11643287f + u2 * (0.05265332f + u2 * -0.01172120f)))));
    b = ay > ax ? 1.57079633f - b : b;
    b = p.x < 0.0f ? 3.14159265f - b : b;
    b = p.y < 0.0f ? -b : b;
    const float c0 = (6.28318531f - b) * c.col_scale;
    const float cf = floorf(c0), fc = c0 - cf;
    ok = ok && fc >= mc && fc <= 1.0f - mc && cf >= 0.0f && cf < c.two_h;
    col = (int)(ok ? cf : 0.0f);
  }
  const bool live = valid && finite;            // the point can have a cell at all
  const bool dec = live && c.fast && ok;        // ... and the estimate decides it
  const int row = rfl >= 0 ? rfl : (rfl == -1 ? 0 : -1);
  col = col >= c.H ? col - c.H : col;
  const bool in = row >= 0 && row < c.NS && col >= 0 && col < c.H;
  *valid_out = valid;
  *cell_out = (dec && in) ? col + row * c.H : -1;
  return !live || dec;
}
// the margins of ip_point_quick (cells) for this sensor
DEV_INLINE void ip_quick_margins(const DevCtx& d, float* mr, float* mc) {
  *mr = fmaxf(0.005f, 8e-6f * 57.29577951f * (float)d.inv_res_y + 1e-5f);
  *mc = fmaxf(0.02f, 8e-6f * 57.29577951f * (float)d.inv_res_x + 8e-7f * (float)d.H);
}

// the ground test of two vertically adjacent cells and the segmentation's edge predicate: ip_pred.h (host-compilable)
DEV_INLINE bool ip_is_ground(const DevCtx& d, float fx, float fy, float fz) {
  return ip_ground_decide(d.tan_g_lo, d.tan_g_hi, d.P.sensor_mount_ang, d.P.ground_angle_thres, fx, fy, fz);
}

// ---- what the compaction writes (imageProjection.cpp:158-191).  Which cell gets which record is ip_rules.h's; here is the record.  Every pointer is
// already offset to the stream's slot (ip_fused_t hands in the ones it fetched late from the kernel-argument segment); q = the cell's input point. ----
DEV_INLINE bool ip_feasible(const alego_params& P, int size, int n_rows) { return ip_seg_feasible(P.seg_big_num, P.seg_valid_point_num, P.seg_valid_line_num, size, n_rows); }
DEV_INLINE int ip_size_class(const alego_params& P, int size) { return ip_seg_size_class(P.seg_big_num, P.seg_valid_point_num, size); }
DEV_INLINE bool ip_class_feasible(const alego_params& P, int size_class, int n_rows) { return ip_seg_class_feasible(size_class, P.seg_valid_line_num, n_rows); }
DEV_INLINE float ip_point_range(float4 q) { return sqrtf(q.x * q.x + q.y * q.y + q.z * q.z); }   // the range image's value (:99), recomputed from the point
// a kept cell: segmentedCloud, GroundFlag, ColInd, Range at output line `line` (:178-186); `range` where the caller has it in hand
DEV_INLINE void ip_store_kept(float4* seg_pts, uint8_t* seg_ground, int* seg_col, float* seg_range, int line, float4 q, int row, int col, double colfrac, bool ground, float range) {
  seg_pts[line] = make_float4(q.x, q.y, q.z, ip_intensity(row, colfrac));
  seg_ground[line] = ground ? 1 : 0;
  seg_col[line] = col;
  seg_range[line] = range;
}
DEV_INLINE void ip_store_kept(float4* seg_pts, uint8_t* seg_ground, int* seg_col, float* seg_range, int line, float4 q, int row, int col, double colfrac, bool ground) {
  ip_store_kept(seg_pts, seg_ground, seg_col, seg_range, line, q, row, col, colfrac, ground, ip_point_range(q));
}
// an outlier: outlierCloud at its own line (:165-171)
DEV_INLINE void ip_store_outlier(float4* outlier, int line, float4 q, int row, double colfrac) { outlier[line] = make_float4(q.x, q.y, q.z, ip_intensity(row, colfrac)); }
// startRingIndex / endRingIndex of one ring; ring_start / ring_end point at that ring's entries
DEV_INLINE void ip_store_ring(int* ring_start, int* ring_end, int first_line, int next_first_line) { *ring_start = ip_ring_start(first_line); *ring_end = ip_ring_end(next_first_line); }
// kept cells, outliers, feasible segments of the scan; sc = the slot's scalars
DEV_INLINE void ip_store_totals(int* sc, int n_kept, int n_outliers, int n_feasible) { sc[SC_M] = n_kept; sc[SC_NOUT] = n_outliers; sc[SC_NFEAS] = n_feasible; }

// Exclusive scan, in place, of three count tables of n <= 64 * NWS entries each (kept cells, outliers, feasible roots, in output order).  Thread e takes
// entry e: the first NWS wavefronts work, every thread of the workgroup calls.  T = the tables' storage type (sums below its range).  wtot: LDS; it is
// left holding the wavefronts' sums, which ip_scan_total adds up for whoever needs a table's total, until the caller's next barrier.  One barrier
// inside; the caller's next one publishes the tables.
template <int NWS, class T>
DEV_INLINE void ip_scan3(T* c0, T* c1, T* c2, int n, int (*wtot)[NWS]) {
  const int e = threadIdx.x, lane = lane_id(), wave = e >> 6;
  const bool work = e < 64 * NWS, in = e < n;
  T* const c[3] = {c0, c1, c2};
  int v3[3] = {0, 0, 0}, in3[3] = {0, 0, 0};
  if (work) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v3[a] = in ? (int)c[a][e] : 0;
      in3[a] = wave_incl_scan(v3[a]);
      if (lane == 63) wtot[a][wave] = in3[a];
    }
  }
  __syncthreads();
  if (work) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int woff = 0;
#pragma unroll
      for (int w = 0; w < NWS; ++w) if (w < wave) woff += wtot[a][w];
      if (in) c[a][e] = (T)(woff + in3[a] - v3[a]);
    }
  }
}
template <int NWS>
DEV_INLINE int ip_scan_total(const int* wtot_a) {
  int t = 0;
#pragma unroll
  for (int w = 0; w < NWS; ++w) t += wtot_a[w];
  return t;
}

// 16-bit variant for n_scan <= 16 (every such image has < 65536 cells): the parent array takes 2 B/cell (58 KB at 16x1800
// instead of 115 KB), so that two of these workgroups — or one of them and the other stream groups' workgroups — fit a CU;
// under load the kernel's duration is decided by that, not by its instruction count.  LDS has no 16-bit atomics: the union's
// compare-and-swap goes through the aligned 32-bit word (a concurrent change of the other half makes it retry), the
// path-halving stores are plain 16-bit stores (parents only ever decrease, any ancestor is a valid parent).  Component size
// and row mask are accumulated one after the other in the ROOTS' OWN parent entries with 32-bit atomics on the packed
// halves (sizes < 65536 cannot carry into the neighbour; OR is bit-local): 2 B/cell of LDS in total.
DEV_INLINE int ccl16_find(uint16_t* par, int v) {
  int curr = par[v];
  if (curr != v) {
    int prev = v, next;
    while (curr > (next = par[curr])) { par[prev] = (uint16_t)next; prev = curr; curr = next; }
  }
  return curr;
}
// compare-and-swap of entry idx (expect -> val); returns the entry's previous value
DEV_INLINE int ccl16_cas(uint16_t* par, int idx, int expect, int val) {
  unsigned* w = reinterpret_cast<unsigned*>(par) + (idx >> 1);
  const int sh = (idx & 1) * 16;
  unsigned old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (true) {
    const int cur = (int)((old >> sh) & 0xFFFFu);
    if (cur != expect) return cur;
    const unsigned nw = (old & ~(0xFFFFu << sh)) | ((unsigned)val << sh);
    const unsigned got = atomicCAS(w, old, nw);
    if (got == old) return expect;
    old = got;
  }
}
DEV_INLINE void ccl16_union(uint16_t* par, int a, int b) {
  int ra = ccl16_find(par, a), rb = ccl16_find(par, b);
  bool repeat;
  do {
    repeat = false;
    if (ra != rb) {
      int ret;
      if (ra < rb) { if ((ret = ccl16_cas(par, rb, rb, ra)) != rb) { rb = ret; repeat = true; } }
      else { if ((ret = ccl16_cas(par, ra, ra, rb)) != ra) { ra = ret; repeat = true; } }
    }
  } while (repeat);
}

#endif
