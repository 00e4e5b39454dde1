// alego_api.hip — host side of the C ABI (include/alego_mi355x.h): HBM allocation, the
// per-handle HIP stream, kernel sequencing and the nodelet-shaped entry points.
// No numerics live here and there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/alego_mi355x.h"
#include "api_gate.h"
#include "dev_common.h"
#include "dev_copy.h"
#include "dev_mem.h"
#include "front_end.h"
#include "lm_ctx.h"
#include "lm_host.h"
#include "merge_math.h"
#include "nn_rules.h"
#include "thin_math.h"
#include "edt_math.h"
#include "occ_math.h"
#include "loop_ctx.h"
#include "pgraph.h"
#include "prof.h"
#include "reg_cov_math.h"
#include "reloc.h"
#include "stream_plan.h"
#include "voxel.h"

thread_local Profiler* g_prof = nullptr;

// A handle drives one HIP stream per stream group and, where the process's hardware queues leave room, a second one per group for
// LaserMapping; the HIP runtime maps streams onto those queues, and streams that share a queue serialise.  stream_plan.h fits the number of
// streams to the queues (alego_stream_plan reports the choice).  How many queues a process opens is the host's setting
// (include/alego_mi355x.h): the library reads GPU_MAX_HW_QUEUES and never writes the environment.

struct alego_handle {
  std::recursive_mutex host_lock;   // alego_handle_lock / alego_handle_unlock: for hosts that drive ONE handle from several threads (the three nodelets)
  alego_params P;
  int device = 0;
  hipStream_t stream = nullptr;       // = streams[0]
  // Slots are split into contiguous groups of `gsize`; each group has its own HIP stream (and its own VoxelGrid scratch in
  // LmHost), so the latency-bound kernels of one group overlap with the kernels of the others.  Slots never interact.
  std::vector<hipStream_t> streams;
  int gsize = 1;
  // alego_batch_run: LaserMapping of scan k runs on a second HIP stream of the group (back[g]) while the group's front end (ImageProjection,
  // feature extraction, LaserOdometry — none of which reads anything LaserMapping writes) already works on scans k + 1, k + 2.  lm_stage
  // hands a scan over (odometry + the three clouds, double-buffered by scan parity); ev_back[g][p] = LaserMapping of the last scan of parity p done.
  bool lm_async = false;
  std::vector<hipStream_t> back;
  std::vector<hipEvent_t> ev_stage, ev_back;   // [group][2]
  std::vector<long> grp_scans;                  // scans handed over per group
  DevCtx d;
  DevPool mem;                 // every device block the handle itself owns
  std::string err;
  std::vector<long> lo_scans;  // LO steps enqueued per slot (the first one only initialises, laserOdometry.cpp:316-324)
  LmHost* lm = nullptr;
  Profiler prof;
  int ip_fast_capable = 0;  // which of ip_project's table fast paths this geometry supports
  bool replay_assigned = false;
  // alego_stream_run: look-ahead lanes
  bool stream_mode = false;
  int lanes = 0;               // W: lanes per set (slots 1 .. W and W + 1 .. 2 W)
  int pose_slot = 0;           // slot holding the poses of the last processed scan of slot 0 (its lane)
  int last_lane = -1;          // lane of the previous scan (LaserOdometry's surf_last_ / corner_last_)
  std::vector<double> imu_last_stamp;   // per slot: stamp of the newest IMU sample (alego_lo_push_imu wants them non-decreasing)
  int next_set = 0;            // lane set the next group of scans uses (the other one still holds the previous scan's features)
  hipStream_t s_lo = nullptr, s_lm = nullptr;   // streams alego_stream_setup created itself (the handle's front and back stream come first)
  hipStream_t sB = nullptr, sC = nullptr;       // the streams LaserOdometry and LaserMapping of a look-ahead stream run on
  StreamPlan plan = {1, 1, 0, STREAM_PLAN_DEFAULT_QUEUES};
  std::vector<hipEvent_t> ev_pool;
  size_t ev_next = 0;
  bool map_on = false;         // alego_map_enable: the key-frame archive exists
  LcCtx* lc = nullptr;         // alego_loop_search: detection / chunk scratch, allocated by the first call and kept
  bool graph_on = false;       // alego_graph_enable: the key-pose graph exists
  PgCtx* pg = nullptr;         // alego_graph_optimize: chunk scratch, allocated by the first call and kept
  RlCtx* rl = nullptr;         // alego_reloc_enable: map / query descriptors; search scratch allocated by the first call and kept
};

namespace {

#define HIP_TRY(h, call)                                                                       \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
      return ALEGO_ERR_HIP;                                                                    \
    }                                                                                          \
  } while (0)

template <class T>
int dalloc(alego_handle* h, T** p, size_t count, bool zero = true) {
  const hipError_t e = h->mem.get(p, count, zero);
  if (e != hipSuccess) { h->err = std::string("device allocation: ") + hipGetErrorString(e); return ALEGO_ERR_HIP; }
  return 0;
}

DevCtx view(const alego_handle* h, int slot0, int n) {
  DevCtx d = h->d;
  d.slot0 = slot0;
  d.n_launch = n;
  return d;
}

hipStream_t stream_of(const alego_handle* h, int slot) { return h->streams[slot / h->gsize]; }
// every stream of the handle, in the order a wait for all of them visits: front, back, look-ahead
std::vector<hipStream_t> all_streams(const alego_handle* h) {
  std::vector<hipStream_t> v(h->streams);
  v.insert(v.end(), h->back.begin(), h->back.end());
  for (hipStream_t s : {h->s_lo, h->s_lm}) if (s) v.push_back(s);
  return v;
}

int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

// LaserMapping work still in flight on the groups' back streams (alego_batch_run without sync): every entry point that reads or writes
// LaserOdometry / LaserMapping state waits for it first — per-slot calls for their own group's back stream (check_slot), whole-handle
// calls (alego_lo_process, alego_lm_process, alego_dist_*) for all of them; alego_stream_run runs LaserMapping on the back stream itself and
// orders its streams behind it with events.  A handle without back streams (stream_plan.h) has nothing to wait for.
void drain_back(alego_handle* h, int slot = -1) {
  if (slot >= 0 && !h->back.empty()) { (void)dev_wait(h->back[std::min<size_t>((size_t)(slot / h->gsize), h->back.size() - 1)]); return; }
  (void)dev_wait(h->back);
}
// the per-slot wait: the slot exists and, unless the caller keeps the back stream running (it says why), its group's back stream is drained
enum BackStream { BACK_DRAINED, BACK_KEPT_RUNNING };
int check_slot(alego_handle* h, int slot, BackStream back = BACK_DRAINED) {
  if (slot < 0 || slot >= h->d.n_slots) { h->err = "slot out of range"; return ALEGO_ERR_ARG; }
  if (back == BACK_DRAINED) drain_back(h, slot);
  return 0;
}
// behind everything already queued on every stream group: the host waits for all the handle's streams, front, back and look-ahead
#define WAIT_ALL(h) do { if (int r_ = DevTry(__func__, &(h)->err).wait(all_streams(h))) return r_; } while (0)

// ---- the gate (api_gate.h has the order of checks and the list rules) --------------------------------------------------------------
// Opened on the first line of every entry point that takes a handle: a null handle is refused; otherwise the handle's device is current and
// every ALEGO_LAUNCH of this thread is timed into the handle's own profiler until the call returns.  It nests (an entry point may call
// another), never synchronises and never allocates.  Between calls g_prof is null: nothing outlives the handle it points into.
struct Gate {
  Profiler* const prev;
  explicit Gate(alego_handle* h) : prev(g_prof) { if (h) { (void)hipSetDevice(h->device); timed_into(&h->prof); } }
  ~Gate() { timed_into(prev); }
  static void timed_into(Profiler* p) { g_prof = p; }
};
#define ALEGO_GATE(h) const Gate gate_(h); if (!(h)) return ALEGO_ERR_ARG
#define ALEGO_GATE_SLOT(h, slot) ALEGO_GATE(h); if (int r_ = check_slot(h, slot)) return r_   // a per-slot call: the gate, then the per-slot wait

// The state a call needs, checked in the order of the bits; the texts are those the calls have always given.
enum Need : unsigned {
  NOT_STREAM_MODE = 1u << 0,   // not after alego_stream_setup
  MAPPING         = 1u << 1,   // a localising handle owns no key frames of its own: the calls that read, write or archive them refuse
  LOCALISING      = 1u << 2,   // alego_loc_enable / alego_loc_enable_from_map has run ...
  LOCALISING_SEED = 1u << 3,   // ... the same for alego_reloc_enable, whose text names the first of the two only
  UNUSED_HANDLE   = 1u << 4,   // no archive, no graph, no scan run yet in any slot
  ARCHIVE         = 1u << 5,   // alego_map_enable has run ...
  ARCHIVE_FIRST   = 1u << 6,   // ... the same for an *_enable that builds on it ("alego_map_enable first")
  GRAPH           = 1u << 7,   // alego_graph_enable has run
  APPEARANCE      = 1u << 8,   // alego_loop_appearance_enable has run
  RELOCALISATION  = 1u << 9,   // alego_reloc_enable has run
};
int gate_need(alego_handle* h, const char* what, unsigned need) {
  auto refuse = [&](const char* why) { h->err = std::string(what) + ": " + why; return ALEGO_ERR_ARG; };
  const bool localising = h->lm && lm_host_localising(h->lm);
  if ((need & NOT_STREAM_MODE) && h->stream_mode) return refuse("not available with alego_stream_setup");
  if ((need & MAPPING) && localising) return refuse("not available on a localising handle (alego_loc_enable)");
  if ((need & LOCALISING) && !localising) return refuse("the handle does not localise (alego_loc_enable / alego_loc_enable_from_map)");
  if ((need & LOCALISING_SEED) && !localising) return refuse("the handle does not localise (alego_loc_enable)");
  if (need & UNUSED_HANDLE) {
    if (h->map_on || h->graph_on) return refuse("the key-frame archive / key-pose graph belong to a mapping handle");
    bool used = false;
    for (long v : h->lo_scans) used = used || v != 0;
    for (long v : h->grp_scans) used = used || v != 0;
    if (used) return refuse("call it before the first scan of any slot");
  }
  if ((need & ARCHIVE) && !h->map_on) return refuse("the key-frame archive is off (alego_map_enable)");
  if ((need & ARCHIVE_FIRST) && !h->map_on) return refuse("the key-frame archive is off (alego_map_enable first)");
  if ((need & GRAPH) && !h->graph_on) return refuse("the key-pose graph is off (alego_map_enable, then alego_graph_enable)");
  if ((need & APPEARANCE) && !loop_app_enabled(h->rl)) return refuse("the appearance search is off (alego_map_enable, then alego_loop_appearance_enable)");
  if ((need & RELOCALISATION) && !reloc_enabled(h->rl)) return refuse("relocalisation is off (alego_loc_enable, then alego_reloc_enable)");
  return 0;
}

}  // namespace

extern "C" {

// These read the handle's host fields only: they stay outside the gate and touch no device state.
int alego_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int alego_params_sizeof(void) { return (int)sizeof(alego_params); }
int alego_handle_lock(alego_handle* h) { if (!h) return ALEGO_ERR_ARG; h->host_lock.lock(); return 0; }
int alego_handle_unlock(alego_handle* h) { if (!h) return ALEGO_ERR_ARG; h->host_lock.unlock(); return 0; }
const char* alego_last_error(const alego_handle* h) { return h ? h->err.c_str() : "null handle"; }
void* alego_stream(alego_handle* h) { return h ? (void*)h->stream : nullptr; }
int alego_stream_groups(const alego_handle* h, int* slots_per_group) {
  if (!h) return ALEGO_ERR_ARG;
  if (slots_per_group) *slots_per_group = h->gsize;
  return (int)h->streams.size();
}

int alego_stream_plan(const alego_handle* h, int out[4]) {
  if (!h || !out) return ALEGO_ERR_ARG;
  out[0] = (int)h->streams.size(); out[1] = h->gsize; out[2] = h->lm_async ? 1 : 0; out[3] = h->plan.queues;
  return 0;
}

int alego_create(const alego_params* params, int device, int n_slots, int ring_len, alego_handle** out) {
  if (!params || !out) return ALEGO_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return ALEGO_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ALEGO_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::fprintf(stderr, "alego_create: device %d is %s, this library is built for gfx950 only\n", device, prop.gcnArchName);
    return ALEGO_ERR_NO_DEVICE;
  }
  if (n_slots <= 0) n_slots = 1;
  if (ring_len <= 0) ring_len = 1;
  if (params->n_scan < 1 || params->n_scan > 64 || params->horizon_scan < 64 || params->horizon_scan > 4096) return ALEGO_ERR_ARG;
  if (params->sort_mode != 0 && params->sort_mode != 2) { std::fprintf(stderr, "alego_create: sort_mode %d is an oracle-only setting (0 = (curvature, index) order, 2 = libstdc++ std::sort tie order in the sector sort)\n", params->sort_mode); return ALEGO_ERR_ARG; }
  if (params->deskew_mode != 0 && params->deskew_mode != 1) { std::fprintf(stderr, "alego_create: deskew_mode must be 0 or 1\n"); return ALEGO_ERR_ARG; }
  if (params->deskew_mode && !(params->scan_period > 0)) { std::fprintf(stderr, "alego_create: scan_period must be positive\n"); return ALEGO_ERR_ARG; }
  if (params->kf_cap_surf < 0 || params->kf_cap_outlier < 0) { std::fprintf(stderr, "alego_create: negative key-frame capacity\n"); return ALEGO_ERR_ARG; }
  if (params->recent_keyframe_num > 512) { std::fprintf(stderr, "alego_create: recent_keyframe_num > 512 is not supported\n"); return ALEGO_ERR_ARG; }
  // The feature pick marks up to suppress_radius neighbours on either side of a picked point; the segmented cloud only
  // guarantees the reference's 5-point margin at both ends of a ring (laserOdometry.cpp:124,211-234 index i +- 5 unchecked).
  if (params->suppress_radius < 0 || params->suppress_radius > 5 || params->n_sectors < 1 || params->n_sharp < 0 ||
      params->n_less_sharp < params->n_sharp || params->n_flat < 1) {
    std::fprintf(stderr, "alego_create: feature-pick parameters out of range (0 <= suppress_radius <= 5, n_sectors >= 1, 0 <= n_sharp <= n_less_sharp, n_flat >= 1)\n");
    return ALEGO_ERR_ARG;
  }
  {
    // the feature pick keeps a sector's candidates in registers: 16 lanes x 43 (fe_pick4) or 64 lanes x 12 (fe_pick) elements
    const int sector_max = (params->horizon_scan + params->n_sectors - 1) / params->n_sectors + 2;
    if (sector_max > 64 * 12) {
      std::fprintf(stderr, "alego_create: ceil(horizon_scan / n_sectors) + 2 = %d exceeds the 768 sector elements the feature pick holds\n", sector_max);
      return ALEGO_ERR_ARG;
    }
  }
  alego_handle* h = new alego_handle();
  h->P = *params;
  h->device = device;
  h->lo_scans.assign(n_slots, 0);
  if (hipSetDevice(device) != hipSuccess) { delete h; return ALEGO_ERR_HIP; }
  {
    // stream groups and back streams, fitted to the hardware queues of the process (stream_plan.h); ALEGO_STREAM_GROUPS / ALEGO_LM_ASYNC are explicit requests
    const char *eg = getenv("ALEGO_STREAM_GROUPS"), *ea = getenv("ALEGO_LM_ASYNC");
    h->plan = stream_plan(n_slots, stream_plan_queues(getenv("ALEGO_HW_QUEUES"), getenv("GPU_MAX_HW_QUEUES")),
                          eg ? std::max(atoi(eg), 0) : -1, ea ? (atoi(ea) != 0 ? 1 : 0) : -1);
    h->gsize = h->plan.gsize;
    const int G = h->plan.groups;
    for (int g = 0; g < G; ++g) {
      hipStream_t s = nullptr;
      if (hipStreamCreate(&s) != hipSuccess) { for (hipStream_t t : h->streams) hipStreamDestroy(t); delete h; return ALEGO_ERR_HIP; }
      h->streams.push_back(s);
    }
    h->stream = h->streams[0];
    h->lm_async = h->plan.async != 0;
    if (h->lm_async) {
      for (int g = 0; g < G; ++g) {
        hipStream_t s = nullptr;
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        bool ok = hipStreamCreate(&s) == hipSuccess;
        for (int k = 0; k < 4 && ok; ++k) ok = hipEventCreateWithFlags(&e[k], hipEventDisableTiming) == hipSuccess;
        if (!ok) { h->lm_async = false; break; }
        h->back.push_back(s);
        h->ev_stage.push_back(e[0]); h->ev_stage.push_back(e[1]); h->ev_back.push_back(e[2]); h->ev_back.push_back(e[3]);
      }
      h->grp_scans.assign(G, 0);
    }
  }
  DevCtx& d = h->d;
  std::memset(&d, 0, sizeof(d));
  d.P = *params;
  d.n_slots = n_slots; d.ring_len = ring_len; d.slot0 = 0; d.n_launch = n_slots;
  d.fs_cur = d.fs_last = -1;
  d.NS = params->n_scan; d.H = params->horizon_scan; d.N = d.NS * d.H; d.Pcap = d.N;
  d.cap_sharp = params->n_sharp * params->n_sectors;
  d.cap_lsharp = params->n_less_sharp * params->n_sectors;
  d.cap_flat = params->n_flat * params->n_sectors;
  d.st_stride = d.cap_sharp + d.cap_lsharp + d.cap_flat + d.H;
  d.sin_ax = std::sin(params->seg_alpha_x); d.cos_ax = std::cos(params->seg_alpha_x);  // imageProjection.cpp:269
  d.sin_ay = std::sin(params->seg_alpha_y); d.cos_ay = std::cos(params->seg_alpha_y);
  {
    const double lo = params->sensor_mount_ang - params->ground_angle_thres, hi = params->sensor_mount_ang + params->ground_angle_thres;
    const bool ok = lo > -89.0 && hi < 89.0 && lo < hi;
    d.tan_g_lo = ok ? std::tan(lo * M_PI / 180.0) : std::nan("");
    d.tan_g_hi = ok ? std::tan(hi * M_PI / 180.0) : std::nan("");
  }
  d.h_magic = (unsigned)((1ull << 32) / (unsigned long long)d.H) + 1u;
  d.inv_res_x = 1.0 / params->ang_res_x; d.inv_res_y = 1.0 / params->ang_res_y;
  d.tan_theta = (params->seg_theta > 0.0 && params->seg_theta < 1.5) ? std::tan(params->seg_theta) : std::nan("");
  d.opt_ip_screen = env_int("ALEGO_IP_SCREEN", 1) != 0;
  d.ip_scr = ip_screen_consts(d.sin_ax, d.cos_ax, d.sin_ay, d.cos_ay, d.tan_theta, d.tan_g_lo, d.tan_g_hi, d.opt_ip_screen);
  d.opt_ip_fused = env_int("ALEGO_IP_FUSED", 1) != 0;
  d.opt_ip_half = env_int("ALEGO_IP_HALF", 1) != 0;
  d.opt_cc_fused = env_int("ALEGO_CC_FUSED", 1) != 0;
  d.opt_cc_tile = env_int("ALEGO_CC_TILE", 1) != 0;
  d.opt_ip_band = env_int("ALEGO_IP_BAND", 1) != 0;
  d.opt_fe_pick1 = env_int("ALEGO_FE_PICK1", 0) != 0;
  d.opt_fe_fused = env_int("ALEGO_FE_FUSED", 1) != 0;
  d.opt_fe_cand = env_int("ALEGO_FE_CAND", 0);
  d.opt_fe_span = env_int("ALEGO_FE_SPAN", 0);
  d.opt_lo_box_lds = env_int("ALEGO_LO_BOX_LDS", 1 << 20);
  d.opt_lo_grid = env_int("ALEGO_LO_GRID", 1) != 0;
  d.opt_fo_spin = env_int("ALEGO_FE_SPIN", 0);
  d.opt_fo_pad8 = env_int("ALEGO_FE_PAD8", 0) != 0;
  d.opt_map_merge = env_int("ALEGO_MAP_MERGE", 1) != 0;
  d.opt_lm_total_merge = env_int("ALEGO_LM_TOTAL_MERGE", 1) != 0;
  d.opt_solve_full_eval = env_int("ALEGO_SOLVE_FULL_EVAL", 0) != 0;
  d.fcap[F_SHARP] = d.cap_sharp * d.NS; d.fcap[F_LSHARP] = d.cap_lsharp * d.NS; d.fcap[F_FLAT] = d.cap_flat * d.NS; d.fcap[F_LFLAT] = d.N;
  d.lo_qcap_surf = d.fcap[F_FLAT]; d.lo_qcap_corner = d.fcap[F_SHARP];
  d.lo_box_cap = (d.N + LO_CH - 1) / LO_CH + d.NS;   // boxes never straddle rings: up to one partly filled box per ring
  const size_t B = n_slots, N = d.N, NS = d.NS;
  int rc = 0;
  rc |= dalloc(h, &d.in_pts, B * ring_len * d.Pcap, false);
  rc |= dalloc(h, &d.in_n, B * ring_len);
  rc |= dalloc(h, &d.owner, B * N); rc |= dalloc(h, &d.range_img, B * N); rc |= dalloc(h, &d.flag_img, B * N);
  rc |= dalloc(h, &d.parent, B * N); rc |= dalloc(h, &d.cc_size, B * N); rc |= dalloc(h, &d.cc_rows, B * N);
  rc |= dalloc(h, &d.label_img, B * N); rc |= dalloc(h, &d.cc_label, B * N);
  d.ipb_col = nullptr; d.ipb_off = nullptr;
  if (d.NS > 16 && d.NS <= 64) { rc |= dalloc(h, &d.ipb_col, B * ipb_col_n(d)); rc |= dalloc(h, &d.ipb_off, B * ipb_off_n(d)); }   // the banded mask path (kernels_ipb.hip)
  d.ipf_own = nullptr;
  if (d.NS <= 16 && d.N <= 65535 && (d.H & 1) == 0) rc |= dalloc(h, &d.ipf_own, B * (N / 2), false);
  rc |= dalloc(h, &d.seg_pts, B * N); rc |= dalloc(h, &d.seg_ground, B * N); rc |= dalloc(h, &d.seg_col, B * N);
  rc |= dalloc(h, &d.seg_range, B * N); rc |= dalloc(h, &d.outlier, B * N);
  rc |= dalloc(h, &d.cd, B * N); rc |= dalloc(h, &d.picked0, B * N); rc |= dalloc(h, &d.fe_flag, B * N); rc |= dalloc(h, &d.plabel, B * N);
  rc |= fe_store_alloc(d, B, [&](auto** p, size_t n, bool zero) { return dalloc(h, p, n, zero); });   // the structured arrays (fe_store.h)
  rc |= dalloc(h, &d.scan_stamp, B);
  rc |= dalloc(h, &d.seg_dsk, h->P.deskew_mode ? B * N : 1);
  {  // boundary tables of ip_project's fast path (kernels_ip.hip)
    const double rx = params->ang_res_x, ry = params->ang_res_y;
    std::vector<double> rt(2 * (NS + 6)), ct;
    for (int k = 0; k < (int)NS + 6; ++k) {   // r = k - 3: the vertical angle at which (va + ang_bottom) / ang_res_y + 0.5 == r
      const double phi = (((double)(k - 3) - 0.5) * ry - params->ang_bottom) * M_PI / 180.0;
      rt[2 * k] = std::cos(phi); rt[2 * k + 1] = std::sin(phi);
    }
    d.ip_cmin = (int)std::floor(180.0 / rx) - 2;
    d.ip_ncb = (int)std::floor(540.0 / rx) + 3 - d.ip_cmin;
    ct.resize(2 * (size_t)d.ip_ncb);
    for (int k = 0; k < d.ip_ncb; ++k) {      // raw column c: the horizontal angle at which ha / ang_res_x == c
      const double A = (double)(d.ip_cmin + k) * rx * M_PI / 180.0;
      ct[2 * k] = std::cos(A); ct[2 * k + 1] = std::sin(A);
    }
    double2 *rtd = nullptr, *ctd = nullptr;
    rc |= dalloc(h, &rtd, NS + 6); rc |= dalloc(h, &ctd, (size_t)d.ip_ncb);
    if (!rc) rc = DevTry("alego_create", &h->err, "upload of the projection tables").up(reinterpret_cast<double*>(rtd), rt).up(reinterpret_cast<double*>(ctd), ct);
    d.ip_rowtab = rtd; d.ip_coltab = ctd;
    {  // col / 10000.0 of every column (the fraction of the intensity row + col / 10000.0, imageProjection.cpp:101): one IEEE fp64 division each, done here once
       // instead of ~35 instructions per emitted cell on the device; the sum with the row and the rounding to f32 stay where they were
      std::vector<double> cf(d.H);
      for (int c = 0; c < d.H; ++c) cf[c] = c / 10000.0;
      double* cfd = nullptr;
      rc |= dalloc(h, &cfd, (size_t)d.H);
      if (!rc) rc = DevTry("alego_create", &h->err, "upload of the column table").up(cfd, cf);
      d.ip_colfrac = cfd;
    }
    d.ip_fast = 0;
    if (params->laser_type == ALEGO_LASER_UNIFORM && ry > 1e-3 && std::fabs(((double)NS + 2.5) * ry - params->ang_bottom) < 80.0 && std::fabs(-3.5 * ry - params->ang_bottom) < 80.0) d.ip_fast |= 1;
    if (rx > 1e-3 && std::fabs((double)d.H * rx - 360.0) < 1e-9 && d.ip_ncb < (1 << 20)) d.ip_fast |= 2;
    h->ip_fast_capable = d.ip_fast;
    d.ip_fast &= env_int("ALEGO_IP_FAST", 3);   // tests: 0 forces the reference expressions for every point
  }
  if (rc) { *out = h; int e = ALEGO_ERR_HIP; std::fprintf(stderr, "alego_create: %s\n", h->err.c_str()); alego_destroy(h); *out = nullptr; return e; }
  // r_w_cur_ = identity, pose quaternions = identity (laserOdometry.cpp:46-47)
  // (host images of the arrays, rows taken by the accessors of a context whose arrays are these vectors)
  std::vector<double> st(B * lo_state_n(), 0.0), po(B * PO_W, 0.0);
  std::vector<int> sc0(B * scal_n(), 0), ip0(B * IMP_W, 0);
  DevCtx hd = d;
  hd.lo_state = st.data(); hd.poses = po.data(); hd.scal = sc0.data(); hd.imu_ptr = ip0.data();
  for (int b = 0; b < n_slots; ++b) {
    double* s = lo_state_of(hd, b);
    s[LS_RW + 0] = s[LS_RW + 4] = s[LS_RW + 8] = 1.0;
    for (int k = 0; k < 6; ++k) s[LS_ROT_P + k] = std::nan("");  // no cached rotation yet
    poses_of(hd, b)[PO_ODOM_Q] = 1.0; poses_of(hd, b)[PO_MAP_Q] = 1.0;
    int* sc = scal_of(hd, b);
    sc[SC_CUR] = 1;  // the first scan writes feature buffer 0
    sc[SC_FIRST] = 0x7fffffff; sc[SC_LAST] = -1;   // accumulators of ip_project, re-armed by ip_front
    imu_ptr_of(hd, b)[IMP_LAST] = -1;   // imu_ptr_last_ = -1, imu_ptr_front_ = imu_ptr_last_iter_ = 0 (laserOdometry.cpp:17-19)
  }
  d.seg_lo = h->P.deskew_mode ? d.seg_dsk : d.seg_pts;
  h->imu_last_stamp.assign(B, -1e300);
  if (DevTry("alego_create", &h->err, "initial state upload").up(d.imu_ptr, ip0).up(d.scal, sc0).up(d.lo_state, st).up(d.poses, po)) { std::fprintf(stderr, "%s\n", h->err.c_str()); alego_destroy(h); return ALEGO_ERR_HIP; }
  if (ip_configure(d) != 0 || lo_configure() != 0 || lm_configure() != 0) { h->err = "hipFuncSetAttribute failed"; std::fprintf(stderr, "alego_create: %s\n", h->err.c_str()); alego_destroy(h); return ALEGO_ERR_HIP; }
  h->lm = lm_host_create(h->P, d, n_slots, h->gsize, h->streams, &h->err);
  if (!h->lm) { std::fprintf(stderr, "alego_create: %s\n", h->err.c_str()); alego_destroy(h); return ALEGO_ERR_HIP; }
  *out = h;
  return ALEGO_OK;
}

void alego_destroy(alego_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  (void)dev_wait(all_streams(h));
  if (h->lm) lm_host_destroy(h->lm);
  loop_ctx_destroy(h->lc);
  reloc_ctx_destroy(h->rl);
  graph_ctx_destroy(h->pg);
  h->mem.clear();
  for (hipStream_t s : h->streams) hipStreamDestroy(s);
  for (hipStream_t s : h->back) hipStreamDestroy(s);
  for (hipEvent_t e : h->ev_stage) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->ev_back) (void)hipEventDestroy(e);
  if (h->s_lo) hipStreamDestroy(h->s_lo);
  if (h->s_lm) hipStreamDestroy(h->s_lm);
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  delete h;
}

int alego_synchronize(alego_handle* h) {
  ALEGO_GATE(h);
  WAIT_ALL(h);
  return 0;
}

int alego_batch_load(alego_handle* h, int slot, int ring_pos, const alego_point* pts, int32_t n) {
  ALEGO_GATE(h);
  if (int r = check_slot(h, slot, BACK_KEPT_RUNNING)) return r;   // only the front end's input ring is written: a host-fed batch_load + batch_run(sync = 0) loop keeps its overlap
  if (ring_pos < 0 || ring_pos >= h->d.ring_len || n < 0 || (n > 0 && !pts)) { h->err = "ring_pos / n out of range or null points"; return ALEGO_ERR_ARG; }
  if (n > h->d.Pcap) { h->err = "scan larger than n_scan*horizon_scan"; return ALEGO_ERR_CAPACITY; }
  float4* dst = h->d.in_pts + ((size_t)slot * h->d.ring_len + ring_pos) * h->d.Pcap;
  const hipStream_t S = stream_of(h, slot);
  return DevTry(__func__, &h->err).up(dst, pts, (size_t)n, S).up(h->d.in_n + slot * h->d.ring_len + ring_pos, &n, 1, S).wait(S);
}

int alego_replay_create(alego_handle* h, int n_bags, int bag_len) {
  ALEGO_GATE(h);
  if (n_bags < 1 || bag_len < 1) return ALEGO_ERR_ARG;
  if (h->d.bag_pts) { h->err = "alego_replay_create: the bag store exists already"; return ALEGO_ERR_ARG; }
  float4* pts = nullptr; int* cnt = nullptr; int2* src = nullptr;
  if (dalloc(h, &pts, (size_t)n_bags * bag_len * h->d.Pcap, false) || dalloc(h, &cnt, (size_t)n_bags * bag_len) || dalloc(h, &src, (size_t)h->d.n_slots)) return ALEGO_ERR_HIP;
  h->d.bag_pts = pts; h->d.bag_n = cnt; h->d.bag_src = src; h->d.n_bags = n_bags; h->d.bag_len = bag_len;
  return 0;
}
int alego_replay_load(alego_handle* h, int bag, int scan, const alego_point* pts, int32_t n) {
  ALEGO_GATE(h);
  if (!h->d.bag_pts || bag < 0 || bag >= h->d.n_bags || scan < 0 || scan >= h->d.bag_len || n < 0 || (n > 0 && !pts)) return ALEGO_ERR_ARG;
  if (n > h->d.Pcap) { h->err = "scan larger than n_scan*horizon_scan"; return ALEGO_ERR_CAPACITY; }
  const size_t idx = (size_t)bag * h->d.bag_len + scan;
  return DevTry(__func__, &h->err).up(const_cast<float4*>(h->d.bag_pts) + idx * h->d.Pcap, pts, (size_t)n).up(const_cast<int*>(h->d.bag_n) + idx, &n, 1);
}
int alego_replay_assign(alego_handle* h, int slot, int bag, int start_scan) {
  ALEGO_GATE_SLOT(h, slot);
  if (!h->d.bag_pts || bag < 0 || bag >= h->d.n_bags || start_scan < 0) return ALEGO_ERR_ARG;
  const int2 v = make_int2(bag, start_scan % h->d.bag_len);
  if (int r = DevTry(__func__, &h->err).up(const_cast<int2*>(h->d.bag_src) + slot, &v, 1)) return r;
  h->replay_assigned = true;
  return 0;
}

int alego_stream_setup(alego_handle* h, int bag, int start_scan) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_stream_setup", MAPPING)) return r;
  if (!h->d.bag_pts || bag < 0 || bag >= h->d.n_bags || start_scan < 0) { h->err = "alego_stream_setup: needs alego_replay_create and a valid bag"; return ALEGO_ERR_ARG; }
  if (h->d.n_slots < 3 || h->streams.size() != 1) { h->err = "alego_stream_setup: the handle needs n_slots = 1 + 2 W >= 3 (one stream group)"; return ALEGO_ERR_ARG; }
  if (h->d.traj) { h->err = "alego_stream_setup: the per-scan pose log belongs to the batch path"; return ALEGO_ERR_ARG; }
  if (h->map_on) { h->err = "alego_stream_setup: the key-frame archive belongs to the batch / single-scan paths"; return ALEGO_ERR_ARG; }
  if (h->P.deskew_mode) { h->err = "alego_stream_setup: bags carry no stamps / IMU data; the motion de-skew runs through alego_scan_process / alego_lo_process"; return ALEGO_ERR_ARG; }
  const int W = (h->d.n_slots - 1) / 2;
  if (int r = alego_replay_assign(h, 0, bag, start_scan)) return r;
  for (int set = 0; set < 2; ++set)
    for (int j = 0; j < W; ++j)   // lane j of either set processes scan (start + group base + j)
      if (int r = alego_replay_assign(h, 1 + set * W + j, bag, start_scan + j)) return r;
  {
    // three chains (ImageProjection + feature extraction ahead, LaserOdometry, LaserMapping) on min(3, Q) streams: the handle's front stream, its
    // back stream where it has one (LaserMapping stays there), and only what is missing beyond them.  With fewer than three, LaserOdometry and
    // LaserMapping — one follows the other anyway — share a stream; with one, everything does (the event waits between the chains stay: harmless).
    std::vector<hipStream_t> pool(1, h->streams[0]);
    if (!h->back.empty()) pool.push_back(h->back[0]);
    const size_t want = (size_t)stream_plan_lookahead_streams(h->plan.queues, (int)pool.size());
    for (hipStream_t* own : {&h->s_lo, &h->s_lm}) {
      if (pool.size() >= want) break;
      if (!*own && hipStreamCreate(own) != hipSuccess) { h->err = "alego_stream_setup: hipStreamCreate failed"; return ALEGO_ERR_HIP; }
      pool.push_back(*own);
    }
    if (pool.size() >= 3) { h->sC = h->back.empty() ? pool[2] : pool[1]; h->sB = h->back.empty() ? pool[1] : pool[2]; }
    else h->sB = h->sC = pool.back();
  }
  h->stream_mode = true; h->lanes = W; h->pose_slot = 0; h->last_lane = -1; h->next_set = 0;
  return 0;
}

int alego_stream_run(alego_handle* h, int first_step, int n_scans, int stages, int sync) {
  ALEGO_GATE(h);
  if (!h->stream_mode) { h->err = "alego_stream_run: call alego_stream_setup first"; return ALEGO_ERR_ARG; }
  // (no drain_back: a one-group handle's back stream is sC here, and the three streams start behind each other below — a host wait
  // would only stall a caller that enqueues run after run with sync = 0)
  const int W = h->lanes;
  hipStream_t sA = h->streams[0], sB = h->sB, sC = h->sC;
  auto ev = [&]() -> hipEvent_t {
    if (h->ev_next == h->ev_pool.size()) { hipEvent_t e; (void)hipEventCreateWithFlags(&e, hipEventDisableTiming); h->ev_pool.push_back(e); }
    return h->ev_pool[h->ev_next++];
  };
  h->ev_next = 0;
  // the three streams start behind whatever any of them did before (earlier runs still in flight, host entry points)
  {
    hipEvent_t eb = ev(), ec = ev(), ea = ev();
    HIP_TRY(h, hipEventRecord(eb, sB)); HIP_TRY(h, hipEventRecord(ec, sC));
    HIP_TRY(h, hipStreamWaitEvent(sA, eb, 0)); HIP_TRY(h, hipStreamWaitEvent(sA, ec, 0));
    HIP_TRY(h, hipEventRecord(ea, sA)); HIP_TRY(h, hipStreamWaitEvent(sB, ea, 0)); HIP_TRY(h, hipStreamWaitEvent(sC, ea, 0));
  }
  hipEvent_t lm_done[2] = {nullptr, nullptr};    // LaserMapping has consumed every lane of the set's previous use
  hipEvent_t lo_first_done = nullptr;            // LaserOdometry of the first scan of the previous group (it still reads the last lane of the group before)
  const bool do_lo = (stages & 2) != 0, do_lm = do_lo && (stages & 4);
  int g = 0;
  for (int base = 0; base < n_scans; base += W, ++g) {
    const int w = std::min(W, n_scans - base), set = h->next_set, lane0 = 1 + set * W;
    h->next_set ^= 1;
    // ---- ImageProjection + feature extraction of w scans, one per lane (stream A)
    if (lm_done[set]) HIP_TRY(h, hipStreamWaitEvent(sA, lm_done[set], 0));
    if (lo_first_done) HIP_TRY(h, hipStreamWaitEvent(sA, lo_first_done, 0));
    DevCtx dl = view(h, lane0, w);
    dl.replay_bag = 1;
    const int pos = (int)(((long long)first_step + base) % h->d.bag_len);
    if (stages & 1) launch_ip(dl, pos, false, sA);
    if (do_lo) launch_fe(dl, sA);
    hipEvent_t fe_done = ev();
    HIP_TRY(h, hipEventRecord(fe_done, sA));
    if (!do_lo) { h->pose_slot = lane0 + w - 1; continue; }
    HIP_TRY(h, hipStreamWaitEvent(sB, fe_done, 0));
    for (int j = 0; j < w; ++j) {
      // ---- LaserOdometry of the stream (slot 0) on the features of lane (stream B)
      DevCtx ds = view(h, 0, 1);
      ds.fs_cur = lane0 + j; ds.fs_last = h->last_lane >= 0 ? h->last_lane : lane0 + j;   // (first scan ever: LaserOdometry only initialises)
      launch_lo(ds, sB);
      hipEvent_t lo_done = ev();
      HIP_TRY(h, hipEventRecord(lo_done, sB));
      if (j == 0) lo_first_done = lo_done;
      const bool odom_valid = h->lo_scans[0]++ > 0;
      if (do_lm) {
        // ---- LaserMapping of that scan (stream C)
        HIP_TRY(h, hipStreamWaitEvent(sC, lo_done, 0));
        if (int r = lm_host_enqueue(h->lm, ds, std::vector<char>(1, odom_valid ? 1 : 0), &h->err, sC)) return r;
      }
      h->last_lane = lane0 + j;
      h->pose_slot = lane0 + j;
    }
    hipEvent_t done = ev();
    HIP_TRY(h, hipEventRecord(done, do_lm ? sC : sB));
    lm_done[set] = done;
  }
  HIP_TRY(h, hipGetLastError());
  if (sync) WAIT_ALL(h);
  return 0;
}

// enqueue IP -> FE -> LO -> LM for slots [slot0, slot0+n) on ring position `pos`
static int enqueue_scan(alego_handle* h, int slot0, int n, int pos, int stages, bool want_labels, bool async_lm = false) {
  DevCtx d = view(h, slot0, n);
  d.replay_bag = (stages & ALEGO_REPLAY_BAG) ? 1 : 0;
  hipStream_t S = stream_of(h, slot0);  // [slot0, slot0+n) lies inside one stream group
  static const bool dbg = getenv("ALEGO_DEBUG_SYNC") != nullptr;
  auto chk = [&](const char* what) { if (dbg) { hipError_t e = hipStreamSynchronize(S); fprintf(stderr, "[alego dbg] %s: %s\n", what, hipGetErrorString(e)); } };
  if (stages & 1) { launch_ip(d, pos, want_labels, S); chk("ip"); }
  if (stages & 2) {
    if (d.P.deskew_mode) { launch_lo_deskew(d, S); chk("deskew"); }   // adjustDistortion(segmented_cloud, t1), laserOdometry.cpp:115
    launch_fe(d, S); chk("fe");
    launch_lo(d, S); chk("lo");
    std::vector<char> odom_valid(n);
    for (int i = 0; i < n; ++i) odom_valid[i] = h->lo_scans[slot0 + i]++ > 0;
    if ((stages & 4) && async_lm && h->lm_async) {
      // LaserMapping of this scan on the group's back stream, behind the hand-over kernel on S (lm_host.hip)
      const int g = slot0 / h->gsize;
      hipStream_t B = h->back[g];
      const long k = h->grp_scans[g]++;
      const int par = (int)(k & 1);
      if (int r = lm_host_enqueue_async(h->lm, d, odom_valid, &h->err, S, B, h->ev_stage[g * 2 + par], h->ev_back[g * 2 + par], h->ev_back[g * 2 + (par ^ 1)], k)) return r;
      if (d.traj) launch_traj_log(d, B, lm_host_stage_odom(h->lm), par);
      HIP_TRY(h, hipEventRecord(h->ev_back[g * 2 + par], B));
    } else {
      if (stages & 4) { if (int r = lm_host_enqueue(h->lm, d, odom_valid, &h->err)) return r; }
      if (d.traj) launch_traj_log(d, S);
    }
  }
  HIP_TRY(h, hipGetLastError());
  return 0;
}

int alego_batch_run(alego_handle* h, int first_pos, int n_scans, int stages, int sync) {
  ALEGO_GATE(h);
  if (n_scans < 0) return ALEGO_ERR_ARG;
  const int R = h->d.ring_len;
  if (h->P.deskew_mode && (stages & 2)) { h->err = "alego_batch_run: the motion de-skew needs every scan's stamp (alego_scan_process / alego_lo_process)"; return ALEGO_ERR_ARG; }
  if ((stages & ALEGO_REPLAY_BAG) && (!h->d.bag_pts || !h->replay_assigned)) { h->err = "alego_batch_run: ALEGO_REPLAY_BAG without alego_replay_create / alego_replay_assign"; return ALEGO_ERR_ARG; }
  for (int s = 0; s < n_scans; ++s) {
    int pos;
    if (stages & ALEGO_REPLAY_BAG) {
      pos = (int)(((long long)first_pos + s) % h->d.bag_len);   // every slot adds its own start scan on the device
    } else if ((stages & ALEGO_REPLAY_PINGPONG) && R > 1) {  // 0,1,..,R-1,R-2,..,1,0,1,.. : consecutive scans stay neighbours
      const int period = 2 * (R - 1);
      const int t = ((first_pos + s) % period + period) % period;
      pos = t < R ? t : period - t;
    } else {
      pos = ((first_pos + s) % R + R) % R;
    }
    for (int s0 = 0; s0 < h->d.n_slots; s0 += h->gsize)
      if (int r = enqueue_scan(h, s0, std::min(h->gsize, h->d.n_slots - s0), pos, stages & (7 | ALEGO_REPLAY_BAG), false, /*async_lm=*/true)) return r;
  }
  if (sync) WAIT_ALL(h);
  return 0;
}

static int fetch_pose(alego_handle* h, int slot, alego_pose* odom, alego_pose* map_pose) {
  double po[PO_W], st[LO_STATE_N];
  int sc[SC_COUNT];
  const int pslot = (h->stream_mode && slot == 0) ? h->pose_slot : slot;   // alego_stream_run: the last scan's poses live in its lane
  if (h->stream_mode) WAIT_ALL(h);
  const hipStream_t S = stream_of(h, slot);
  if (int r = DevTry(__func__, &h->err).down(po, poses_of(h->d, pslot), S).down(st, lo_state_of(h->d, slot), S).down(sc, scal_of(h->d, slot), S).wait(S)) return r;
  if (odom) {
    for (int i = 0; i < 3; ++i) odom->t[i] = po[PO_ODOM_T + i];
    for (int i = 0; i < 4; ++i) odom->q[i] = po[PO_ODOM_Q + i];
    for (int i = 0; i < 6; ++i) odom->params[i] = st[LS_PARAMS + i];
    odom->valid = sc[SC_ODOM_VALID];
  }
  if (map_pose) {
    for (int i = 0; i < 3; ++i) map_pose->t[i] = po[PO_MAP_T + i];
    for (int i = 0; i < 4; ++i) map_pose->q[i] = po[PO_MAP_Q + i];
    lm_host_get_params(h->lm, slot, map_pose->params);
    map_pose->valid = sc[SC_ODOM_VALID];
  }
  if (sc[SC_FE_ERR]) { h->err = "feature extraction: a ring's workgroup gave up waiting for the voxel counts of the rings below it (fe_ring_out); the slot's feature clouds are incomplete"; return ALEGO_ERR_HIP; }
  const int lmf = lm_host_get_flags(h->lm, slot);
  if (lmf < 0) { h->err = "LaserMapping device capacity exceeded / launch logic out of sync"; return lmf; }
  return sc[SC_LO_FLAGS] | lmf;
}

int alego_batch_get_pose(alego_handle* h, int slot, alego_pose* odom, alego_pose* map_pose) {
  ALEGO_GATE_SLOT(h, slot);
  return fetch_pose(h, slot, odom, map_pose);
}

int alego_trajectory_enable(alego_handle* h, int32_t capacity_scans) {
  ALEGO_GATE(h);
  if (capacity_scans <= 0) return ALEGO_ERR_ARG;
  if (h->stream_mode) { h->err = "alego_trajectory_enable: not available with alego_stream_setup (the poses of a look-ahead stream live in its lanes)"; return ALEGO_ERR_ARG; }
  if (h->d.traj) { h->err = "alego_trajectory_enable: already enabled"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  double* t = nullptr;
  int* n = nullptr;
  if (dalloc(h, &t, (size_t)h->d.n_slots * capacity_scans * PO_LOG_W) || dalloc(h, &n, (size_t)h->d.n_slots)) return ALEGO_ERR_HIP;
  h->d.traj = t; h->d.traj_n = n; h->d.traj_cap = capacity_scans;
  return 0;
}
int alego_trajectory_get(alego_handle* h, int slot, int32_t first, int32_t n, double* out14) {
  ALEGO_GATE_SLOT(h, slot);
  if (!h->d.traj || first < 0 || n < 0 || (n > 0 && !out14)) return ALEGO_ERR_ARG;
  hipStream_t S = stream_of(h, slot);
  int logged = 0;
  DevTry c(__func__, &h->err);
  if (c.down(&logged, traj_n_of(h->d, slot), 1, S).wait(S)) return c;
  const int have = std::min(logged, h->d.traj_cap);
  if (first > have || n > have - first) { h->err = "alego_trajectory_get: range beyond the scans logged"; return ALEGO_ERR_ARG; }   // (not first + n: it overflows for large arguments)
  if (n > 0 && c.down(out14, traj_of(h->d, slot, first), (size_t)n * PO_LOG_W, S).wait(S)) return c;   // (the guard is the wait's)
  return logged;
}

int alego_batch_get_counts(alego_handle* h, int slot, int32_t* out, int cap) {
  ALEGO_GATE_SLOT(h, slot);
  int sc[SC_COUNT], fc[F_KINDS], sl[SC_COUNT];
  const bool lane = h->stream_mode && slot == 0;   // alego_stream_run: the per-scan counters of the last scan live in its lane (buffer 0)
  const int cslot = lane ? h->pose_slot : slot;
  if (lane) WAIT_ALL(h);
  const hipStream_t S = stream_of(h, slot);
  DevTry c(__func__, &h->err);
  if (c.down(sc, scal_of(h->d, cslot), S).down(sl, scal_of(h->d, slot), S).wait(S)) return c;
  const int cur = lane ? 0 : sc[SC_CUR];  // buffer written by the last processed scan
  if (c.down(fc, feat_cnt_of(h->d, fbuf(cslot, cur)))) return c;
  sc[SC_LO_NSURF] = sl[SC_LO_NSURF]; sc[SC_LO_NCORNER] = sl[SC_LO_NCORNER];   // LaserOdometry's counters belong to the stream's own slot
  int v[16] = {sc[SC_PVALID_OUT], sc[SC_M], sc[SC_NOUT], fc[F_SHARP], fc[F_LSHARP], fc[F_FLAT], fc[F_LFLAT],
               sc[SC_LO_NSURF], sc[SC_LO_NCORNER], 0, 0, 0, 0, 0, 0, 0};  // v[15] = map rebuilds so far
  lm_host_get_counts(h->lm, slot, v + 9);
  for (int i = 0; i < cap && i < 16; ++i) out[i] = v[i];
  return 0;
}

static int download_seg(alego_handle* h, int slot, alego_seg_out* out) {
  const DevCtx& d = h->d;
  int sc[SC_COUNT];
  const hipStream_t S = stream_of(h, slot);
  DevTry c(__func__, &h->err);
  if (c.down(sc, scal_of(d, slot), S).wait(S)) return c;
  const int M = sc[SC_M], NO = sc[SC_NOUT];
  out->m = M; out->n_outlier = NO;
  if (M > out->seg_cap || NO > out->outlier_cap) { h->err = "seg/outlier capacity too small"; return ALEGO_ERR_CAPACITY; }
  const size_t base = (size_t)slot * d.N;
  static_assert(sizeof(out->orientation) == ORI_N * sizeof(float), "alego_seg_out::orientation is an ori row without its padding");
  if (out->seg) c.down(out->seg, d.seg_pts + base, (size_t)M, S);
  if (out->ground) c.down(out->ground, d.seg_ground + base, (size_t)M, S);
  if (out->col) c.down(out->col, d.seg_col + base, (size_t)M, S);
  if (out->range) c.down(out->range, d.seg_range + base, (size_t)M, S);
  if (out->ring_start) c.down(out->ring_start, ring_start_of(d, slot, 0), (size_t)d.NS, S);
  if (out->ring_end) c.down(out->ring_end, ring_end_of(d, slot, 0), (size_t)d.NS, S);
  c.down(out->orientation, ori_of(d, slot), S);
  if (out->outlier) c.down(out->outlier, d.outlier + base, (size_t)NO, S);
  if (out->label_image) c.down(out->label_image, d.label_img + base, (size_t)d.N, S);
  return c.wait(S);
}

static int download_feat(alego_handle* h, int slot, alego_feat_out* f) {
  const DevCtx& d = h->d;
  int fc[F_KINDS], M, cur;
  const hipStream_t S = stream_of(h, slot);
  DevTry c(__func__, &h->err);
  if (c.down(&cur, scal_of(d, slot) + SC_CUR, 1)) return c;
  if (c.down(fc, feat_cnt_of(d, fbuf(slot, cur)), S).down(&M, scal_of(d, slot) + SC_M, 1, S).wait(S)) return c;
  f->n_sharp = fc[F_SHARP]; f->n_less_sharp = fc[F_LSHARP]; f->n_flat = fc[F_FLAT]; f->n_less_flat = fc[F_LFLAT];
  if (fc[F_SHARP] > f->sharp_cap || fc[F_LSHARP] > f->less_sharp_cap || fc[F_FLAT] > f->flat_cap || fc[F_LFLAT] > f->less_flat_cap) { h->err = "feature capacity too small"; return ALEGO_ERR_CAPACITY; }
  alego_point* dst[F_KINDS] = {f->sharp, f->less_sharp, f->flat, f->less_flat};
  for (int k = 0; k < F_KINDS; ++k)
    if (dst[k]) c.down(dst[k], feat_of(d, k, fbuf(slot, cur)), (size_t)fc[k], S);
  if (f->point_label) c.down(f->point_label, d.plabel + (size_t)slot * d.N, (size_t)M, S);
  return c.wait(S);
}

int alego_ip_process(alego_handle* h, const alego_scan_in* in, alego_seg_out* out) {
  ALEGO_GATE(h);
  if (!in || !out) return ALEGO_ERR_ARG;
  if (int r = alego_batch_load(h, 0, 0, in->pts, in->n)) return r;
  const DevCtx d = view(h, 0, 1);
  launch_ip(d, 0, out->label_image != nullptr, h->stream);
  HIP_TRY(h, hipGetLastError());
  out->stamp = in->stamp;   // /segmented_cloud and /seg_info carry the input's stamp (imageProjection.cpp:318-336)
  return download_seg(h, 0, out);
}

int alego_lo_process(alego_handle* h, const alego_seg_out* in, alego_feat_out* feat, alego_pose* odom) {
  ALEGO_GATE(h);
  if (!in) return ALEGO_ERR_ARG;
  drain_back(h);
  const DevCtx& d = h->d;
  const int slot = 0;   // the single-scan entry points work on slot 0
  if (in->m < 0 || in->m > d.N) { h->err = "segmented cloud larger than n_scan*horizon_scan"; return ALEGO_ERR_CAPACITY; }
  if (!in->ring_start || !in->ring_end || (in->m > 0 && (!in->seg || !in->ground || !in->col || !in->range))) { h->err = "alego_lo_process: null input array"; return ALEGO_ERR_ARG; }
  const size_t M = in->m;
  const hipStream_t S = h->stream;
  DevTry c(__func__, &h->err);
  c.up(d.seg_pts, in->seg, M, S).up(d.seg_ground, in->ground, M, S).up(d.seg_col, in->col, M, S).up(d.seg_range, in->range, M, S);
  c.up(ring_start_of(d, slot, 0), in->ring_start, (size_t)d.NS, S).up(ring_end_of(d, slot, 0), in->ring_end, (size_t)d.NS, S).up(scal_of(d, slot) + SC_M, &in->m, 1, S);
  c.up(ori_of(d, slot), in->orientation, S);       // seg_info's start / end orientation: adjustDistortion reads them
  if (c.up(d.scan_stamp + slot, &in->stamp, 1, S)) return c;
  if (h->map_on && lm_host_map_mark_stamped(h->lm, 0, S)) { h->err = "alego_lo_process: upload failed"; return ALEGO_ERR_HIP; }
  if (c.wait(S)) return c;
  if (int r = enqueue_scan(h, 0, 1, 0, 2, false)) return r;
  if (feat) { if (int r = download_feat(h, 0, feat)) return r; }
  const int r = fetch_pose(h, 0, odom, nullptr);
  return r < 0 ? r : (r & 7);
}

int alego_lm_process(alego_handle* h, const alego_point* corner_last, int32_t n_corner, const alego_point* surf_last,
                     int32_t n_surf, const alego_point* outlier, int32_t n_outlier, const alego_pose* odom, alego_pose* map_pose) {
  ALEGO_GATE(h);
  if (!odom) return ALEGO_ERR_ARG;
  drain_back(h);
  return lm_host_process_host(h->lm, h->d, corner_last, n_corner, surf_last, n_surf, outlier, n_outlier, odom, map_pose, &h->err);
}

int alego_scan_process(alego_handle* h, int slot, const alego_scan_in* in, int stages, alego_seg_out* seg,
                       alego_feat_out* feat, alego_pose* odom, alego_pose* map_pose) {
  ALEGO_GATE_SLOT(h, slot);
  if (!in) return ALEGO_ERR_ARG;
  if (int r = alego_batch_load(h, slot, 0, in->pts, in->n)) return r;
  const hipStream_t S = stream_of(h, slot);
  DevTry c(__func__, &h->err);
  if (c.up(h->d.scan_stamp + slot, &in->stamp, 1, S)) return c;
  if (h->map_on && lm_host_map_mark_stamped(h->lm, slot, S)) { h->err = "alego_scan_process: upload failed"; return ALEGO_ERR_HIP; }
  if (c.wait(S)) return c;   // (`in` is the caller's)
  if (int r = enqueue_scan(h, slot, 1, 0, stages, seg && seg->label_image)) return r;
  if (seg) { if (int r = download_seg(h, slot, seg)) return r; seg->stamp = in->stamp; }
  if (feat && (stages & 2)) { if (int r = download_feat(h, slot, feat)) return r; }
  return fetch_pose(h, slot, odom, map_pose);
}

int alego_set_lo_params(alego_handle* h, int slot, const double* p6) {
  ALEGO_GATE_SLOT(h, slot);
  const hipStream_t S = stream_of(h, slot);
  return DevTry(__func__, &h->err).up(lo_state_of(h->d, slot) + LS_PARAMS, p6, 6, S).wait(S);
}
int alego_set_lm_params(alego_handle* h, int slot, const double* p6) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_set_params(h->lm, slot, p6, &h->err);
}

// /undistorted (laserOdometry.cpp:56,718-725): the de-skewed segmented cloud of the slot's last scan
int alego_lo_get_undistorted(alego_handle* h, int slot, alego_point* out, int32_t cap) {
  ALEGO_GATE_SLOT(h, slot);
  if (!h->P.deskew_mode) { h->err = "alego_lo_get_undistorted: deskew_mode is 0 (adjustDistortion is not run: laserOdometry.cpp:115)"; return ALEGO_ERR_ARG; }
  if (cap < 0 || (cap > 0 && !out)) return ALEGO_ERR_ARG;
  int M = 0;
  const hipStream_t S = stream_of(h, slot);
  DevTry c(__func__, &h->err);
  if (c.down(&M, scal_of(h->d, slot) + SC_M_DSK, 1, S).wait(S)) return c;   // lo_deskew's own count, not SC_M
  if (M > cap) return ALEGO_ERR_CAPACITY;
  if (M > 0 && c.down(out, h->d.seg_dsk + (size_t)slot * h->d.N, (size_t)M)) return c;   // (M < 0 cannot be a count)
  return M;
}

// The standalone LaserOdometry node publishes /odom/lidar as /odom -> /base_link: tf_o2b = tf_o2l * tf_b2l^-1, quaternion from its rotation block
// (LO.cpp:588-608; the nodelet publishes /odom -> /laser as it is, laserOdometry.cpp:513-529).  Host arithmetic only (a publishing convention, not part
// of the hot path): general 4 x 4 inverse by Gauss-Jordan with partial pivoting, Eigen's Quaterniond(Matrix3d) (largest-diagonal branch selection).
int alego_pose_o2b(const alego_pose* o2l, const double* tf_b2l, alego_pose* o2b) {
  if (!o2l || !tf_b2l || !o2b) return ALEGO_ERR_ARG;
  double A[4][8];
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { A[i][j] = tf_b2l[4 * i + j]; A[i][4 + j] = i == j ? 1.0 : 0.0; }
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    for (int r = c + 1; r < 4; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
    if (!(std::fabs(A[piv][c]) > 0.0)) return ALEGO_ERR_ARG;   // singular (or NaN) mount transform
    if (piv != c) for (int j = 0; j < 8; ++j) std::swap(A[piv][j], A[c][j]);
    const double inv = 1.0 / A[c][c];
    for (int j = 0; j < 8; ++j) A[c][j] *= inv;
    for (int r = 0; r < 4; ++r) if (r != c) { const double f = A[r][c]; if (f != 0.0) for (int j = 0; j < 8; ++j) A[r][j] -= f * A[c][j]; }
  }
  const double w = o2l->q[0], x = o2l->q[1], y = o2l->q[2], z = o2l->q[3];
  const double T[4][4] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), o2l->t[0]},
                          {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), o2l->t[1]},
                          {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), o2l->t[2]},
                          {0, 0, 0, 1}};
  double M[4][4];
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double acc = 0; for (int k = 0; k < 4; ++k) acc += T[i][k] * A[k][4 + j]; M[i][j] = acc; }
  *o2b = *o2l;
  for (int i = 0; i < 3; ++i) o2b->t[i] = M[i][3];
  double q[4];   // w, x, y, z
  double t = M[0][0] + M[1][1] + M[2][2];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0); q[0] = 0.5 * t; t = 0.5 / t;
    q[1] = (M[2][1] - M[1][2]) * t; q[2] = (M[0][2] - M[2][0]) * t; q[3] = (M[1][0] - M[0][1]) * t;
  } else {
    int i = 0;
    if (M[1][1] > M[0][0]) i = 1;
    if (M[2][2] > M[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(M[i][i] - M[j][j] - M[k][k] + 1.0);
    q[1 + i] = 0.5 * t; t = 0.5 / t;
    q[0] = (M[k][j] - M[j][k]) * t; q[1 + j] = (M[j][i] + M[i][j]) * t; q[1 + k] = (M[k][i] + M[i][k]) * t;
  }
  for (int i = 0; i < 4; ++i) o2b->q[i] = q[i];
  return ALEGO_OK;
}

// imuHandler (laserOdometry.cpp:761-802): the per-sample trigonometry here, ring bookkeeping + dead reckoning on the device
int alego_lo_push_imu(alego_handle* h, int slot, const alego_imu* smp, int32_t n) {
  ALEGO_GATE_SLOT(h, slot);
  if (n < 0 || (n > 0 && !smp)) return ALEGO_ERR_ARG;
  if (n == 0) return 0;
  std::vector<double> pre((size_t)n * 7);
  double prev = h->imu_last_stamp[slot];
  for (int i = 0; i < n; ++i) {
    const alego_imu& m = smp[i];
    if (!(m.stamp >= prev)) { h->err = "alego_lo_push_imu: IMU stamps must not decrease"; return ALEGO_ERR_ARG; }
    prev = m.stamp;
    const double qw = m.orientation[0], qx = m.orientation[1], qy = m.orientation[2], qz = m.orientation[3];
    // tf::Matrix3x3(ori).getRPY(roll, pitch, yaw) (:765-767)  [upstream tf: setRotation + getEulerYPR, solution 1]
    double roll, pitch, yaw;
    {
      const double dd = qx * qx + qy * qy + qz * qz + qw * qw, sc = 2.0 / dd;
      const double xs = qx * sc, ys = qy * sc, zs = qz * sc;
      const double wx = qw * xs, wy = qw * ys, wz = qw * zs, xx = qx * xs, xy = qx * ys, xz = qx * zs, yy = qy * ys, yz = qy * zs, zz = qz * zs;
      const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
      if (std::fabs(m20) >= 1) {
        yaw = 0;
        const double delta = std::atan2(m21, m22);
        if (m20 < 0) { pitch = M_PI / 2.0; roll = delta; } else { pitch = -M_PI / 2.0; roll = delta; }
      } else {
        pitch = -std::asin(m20);
        roll = std::atan2(m21 / std::cos(pitch), m22 / std::cos(pitch));
        yaw = std::atan2(m10 / std::cos(pitch), m00 / std::cos(pitch));
      }
    }
    const double acc_x = m.linear_acceleration[0] + 9.81 * std::sin(pitch);                      // :768-770
    const double acc_y = m.linear_acceleration[1] - 9.81 * std::cos(pitch) * std::sin(roll);
    const double acc_z = m.linear_acceleration[2] - 9.81 * std::cos(pitch) * std::cos(roll);
    // Eigen::Quaternionf(w, x, y, z).toRotationMatrix() * Vector3f(acc) in f32 (:785-786)
    const float w = (float)qw, x = (float)qx, y = (float)qy, z = (float)qz;
    const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}};
    const float a[3] = {(float)acc_x, (float)acc_y, (float)acc_z};
    double* o = &pre[(size_t)i * 7];
    o[0] = m.stamp; o[1] = roll; o[2] = pitch; o[3] = yaw;
    for (int k = 0; k < 3; ++k) o[4 + k] = (double)(R[k][0] * a[0] + (R[k][1] * a[1] + R[k][2] * a[2]));
  }
  DevPool T;   // temporaries of this call
  double* dp;
  HIP_TRY(h, T.get(&dp, pre.size(), false));
  hipStream_t S = stream_of(h, slot);
  DevTry c(__func__, &h->err);
  if (c.up(dp, pre, S)) return c;
  launch_lo_imu_push(h->d, slot, dp, n, S);
  if (c.wait(S)) return c;
  h->imu_last_stamp[slot] = prev;
  return 0;
}

int alego_profile_enable(alego_handle* h, int on) {
  ALEGO_GATE(h);
  WAIT_ALL(h);
  h->prof.reset();
  h->prof.on = on != 0;
  return 0;
}

int alego_profile_report(alego_handle* h, char* names, int names_cap, double* total_ms, int* launches, int cap) {
  ALEGO_GATE(h);
  WAIT_ALL(h);
  Profiler& P = h->prof;
  const int nk = (int)P.names.size();
  std::vector<double> tot(nk, 0.0);
  std::vector<int> cnt(nk, 0);
  for (auto& r : P.recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { tot[r.id] += ms; cnt[r.id]++; }
  }
  std::string joined;
  for (int i = 0; i < nk; ++i) { if (i) joined += ";"; joined += P.names[i]; }
  if ((int)joined.size() + 1 > names_cap || nk > cap) { h->err = "profile_report: buffers too small"; return ALEGO_ERR_CAPACITY; }
  std::memcpy(names, joined.c_str(), joined.size() + 1);
  for (int i = 0; i < nk; ++i) { total_ms[i] = tot[i]; launches[i] = cnt[i]; }
  return nk;
}

int alego_debug_voxel(alego_handle* h, const alego_point* pts, int n, float leaf, alego_point* out, int cap) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && !pts)) return ALEGO_ERR_ARG;
  DevPool T;   // temporaries of this call
  float4 *din = nullptr, *dout = nullptr;
  int* cnt = nullptr;
  const int c = n > 0 ? n : 1;
  HIP_TRY(h, T.get(&din, (size_t)c, false)); HIP_TRY(h, T.get(&dout, (size_t)c, false)); HIP_TRY(h, T.get(&cnt, 2, false));
  const int hc[2] = {n, 0};
  DevTry t(__func__, &h->err);
  if (t.up(cnt, hc).up(din, pts, (size_t)n)) return t;
  VoxJob job{din, cnt, dout, cnt + 1, nullptr, leaf, c, c, nullptr, 0};
  VoxCtx V;
  if (vox_create(&V, &job, 1, &h->err)) return ALEGO_ERR_HIP;
  int rc = vox_run(V, h->stream, &h->err);
  int nout = 0;
  t.wait(h->stream).down(&nout, cnt + 1, 1);
  if (t.ok() && rc == 0 && nout > cap) { h->err = "debug_voxel: output capacity"; rc = ALEGO_ERR_CAPACITY; }
  if (rc == 0) t.down(out, dout, (size_t)nout);
  vox_destroy(&V);
  if (t) return t;
  return rc ? rc : nout;
}

int alego_debug_math(alego_handle* h, int mode, const float* a, const float* b, float* out, int n) {
  ALEGO_GATE(h);
  if (n < 0 || mode < 0 || mode > 3 || (n > 0 && (!a || !out || (mode < 2 && !b)))) return ALEGO_ERR_ARG;
  if (n == 0) return 0;
  DevPool T;   // temporaries of this call
  float *da, *db, *dout;
  HIP_TRY(h, T.get(&da, (size_t)n, false)); HIP_TRY(h, T.get(&db, (size_t)n, false)); HIP_TRY(h, T.get(&dout, (size_t)n, false));
  DevTry c(__func__, &h->err);
  c.up(da, a, (size_t)n);
  if (b) c.up(db, b, (size_t)n);
  if (c) return c;
  // the probe kernel takes (y, x): atan2f(y, x), hypotf(x, y), sinf(y), cosf(y)
  launch_atan2f_probe(da, db, dout, n, mode, h->stream);
  return c.wait(h->stream).down(out, dout, (size_t)n);
}
int alego_debug_atan2f(alego_handle* h, const float* y, const float* x, float* out, int n) { ALEGO_GATE(h); return alego_debug_math(h, 0, y, x, out, n); }

int alego_debug_std_sort(alego_handle* h, const uint32_t* keys, int n, int depth_limit, int32_t* order) {
  ALEGO_GATE(h);
  if (n < 0 || n > 4096 || (n > 0 && (!keys || !order))) return ALEGO_ERR_ARG;
  if (n == 0) return 0;
  DevPool T;   // temporaries of this call
  uint32_t* dk;
  int* dp;
  HIP_TRY(h, T.get(&dk, (size_t)n, false)); HIP_TRY(h, T.get(&dp, (size_t)n, false));
  DevTry c(__func__, &h->err);
  if (c.up(dk, keys, (size_t)n)) return c;
  if (launch_stdsort_probe(dk, n, depth_limit, dp, h->stream)) return ALEGO_ERR_ARG;
  std::vector<int> pos(n), arr(n);
  if (c.wait(h->stream).down(pos, dp)) return c;
  // the device returns where the partition phase left every element; __final_insertion_sort is a stable sort of that arrangement
  for (int i = 0; i < n; ++i) { if (pos[i] < 0 || pos[i] >= n) { h->err = "alego_debug_std_sort: arrangement out of range"; return ALEGO_ERR_HIP; } arr[pos[i]] = i; }
  std::stable_sort(arr.begin(), arr.end(), [&](int a, int b) { return keys[a] < keys[b]; });
  for (int i = 0; i < n; ++i) order[i] = arr[i];
  return 0;
}

int alego_debug_eval_blocks(alego_handle* h, int type, int n, const double* geom13, const double* params6, double* res, double* jac6) {
  ALEGO_GATE(h);
  if (n < 0 || type < 0 || type > 3 || !params6 || (n > 0 && (!geom13 || !res || !jac6))) return ALEGO_ERR_ARG;
  if (n == 0) return 0;
  DevPool T;   // temporaries of this call
  double *dg, *dp, *dr, *dj;
  HIP_TRY(h, T.get(&dg, (size_t)n * 13, false)); HIP_TRY(h, T.get(&dp, 6, false)); HIP_TRY(h, T.get(&dr, (size_t)n, false)); HIP_TRY(h, T.get(&dj, (size_t)n * 6, false));
  DevTry c(__func__, &h->err);
  if (c.up(dg, geom13, (size_t)n * 13).up(dp, params6, 6)) return c;
  launch_dbg_eval_blocks(type, n, dg, dp, dr, dj, h->stream);
  return c.wait(h->stream).down(res, dr, (size_t)n).down(jac6, dj, (size_t)n * 6);
}

int alego_debug_transform_to_start(alego_handle* h, const double* params6, const alego_point* pts, int n, alego_point* out) {
  ALEGO_GATE(h);
  if (n < 0 || !params6 || (n > 0 && (!pts || !out))) return ALEGO_ERR_ARG;
  if (n == 0) return 0;
  DevPool T;   // temporaries of this call
  double* dp;
  float4 *di, *dout;
  HIP_TRY(h, T.get(&dp, 6, false)); HIP_TRY(h, T.get(&di, (size_t)n, false)); HIP_TRY(h, T.get(&dout, (size_t)n, false));
  DevTry c(__func__, &h->err);
  if (c.up(dp, params6, 6).up(di, pts, (size_t)n)) return c;
  launch_dbg_transform_to_start(dp, di, n, dout, h->stream);
  return c.wait(h->stream).down(out, dout, (size_t)n);
}

int alego_debug_check_guards(char* report, int cap) {
  std::string r;
  const int bad = guard_check(&r);
  if (report && cap > 0) { std::strncpy(report, r.c_str(), (size_t)cap - 1); report[cap - 1] = 0; }
  return bad;
}

int alego_debug_set_option(alego_handle* h, const char* name, int value) {
  ALEGO_GATE(h);
  if (!name) return ALEGO_ERR_ARG;
  const std::string s(name);
  DevCtx& d = h->d;
  if (s == "ALEGO_CC_FUSED") d.opt_cc_fused = value != 0;
  else if (s == "ALEGO_IP_FUSED") d.opt_ip_fused = value != 0;
  else if (s == "ALEGO_IP_HALF") d.opt_ip_half = value != 0;
  else if (s == "ALEGO_IP_SCREEN") { d.opt_ip_screen = value != 0; d.ip_scr = ip_screen_consts(d.sin_ax, d.cos_ax, d.sin_ay, d.cos_ay, d.tan_theta, d.tan_g_lo, d.tan_g_hi, d.opt_ip_screen); }
  else if (s == "ALEGO_CC_TILE") d.opt_cc_tile = value != 0;
  else if (s == "ALEGO_IP_BAND") {   // the banded path expects the component statistics at zero between scans (it re-zeroes what it touched); the cc_stats path leaves them set
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemset(d.cc_size, 0, (size_t)d.n_slots * d.N * sizeof(int)));
    HIP_TRY(h, hipMemset(d.cc_rows, 0, (size_t)d.n_slots * d.N * sizeof(unsigned long long)));
    d.opt_ip_band = value != 0;
  }
  else if (s == "ALEGO_FE_PICK1") d.opt_fe_pick1 = value != 0;
  else if (s == "ALEGO_FE_FUSED") d.opt_fe_fused = value != 0;
  else if (s == "ALEGO_FE_CAND") d.opt_fe_cand = value;
  else if (s == "ALEGO_FE_SPAN") d.opt_fe_span = value;
  else if (s == "ALEGO_LO_BOX_LDS") d.opt_lo_box_lds = value;
  else if (s == "ALEGO_LO_GRID") d.opt_lo_grid = value != 0;
  else if (s == "ALEGO_FE_SPIN") d.opt_fo_spin = value;
  else if (s == "ALEGO_SOLVE_FULL_EVAL") d.opt_solve_full_eval = value != 0;
  else if (s == "ALEGO_FE_PAD8") d.opt_fo_pad8 = value != 0;
  else if (s == "ALEGO_FE_ERR_CLEAR") {   // the per-slot reset of the sticky SC_FE_ERR (dev_common.h): value = slot, -1 = every slot; the caller has drained the handle's streams
    if (value < -1 || value >= d.n_slots) return ALEGO_ERR_ARG;
    HIP_TRY(h, hipDeviceSynchronize());
    if (value >= 0) HIP_TRY(h, hipMemset(scal_of(d, value) + SC_FE_ERR, 0, 4));
    else HIP_TRY(h, hipMemset2D(scal_of(d, 0) + SC_FE_ERR, scal_n() * sizeof(int), 0, 4, d.n_slots));
  }
  else if (s == "ALEGO_MAP_MERGE") { if (int r = lm_host_set_map_merge(h->lm, value != 0, &h->err)) return r; d.opt_map_merge = value != 0; }
  else if (s == "ALEGO_LM_TOTAL_MERGE") d.opt_lm_total_merge = value != 0;   // (both sequences leave the same clouds and counts; lm_total_merge's list counters are its own, vox_plan never writes them)
  else if (s == "ALEGO_IP_FAST") d.ip_fast = h->ip_fast_capable & value;
  else if (s == "ALEGO_POKE_GUARD") { HIP_TRY(h, hipMemset(scal_of(d, d.n_slots) + value, 0xFF, 4)); }   // tests of the guard pages: a write `value` ints past the end of an array
  else if (s == "ALEGO_GV_SMALL_MAX") { WAIT_ALL(h); return lm_host_set_gv_small_max(h->lm, value); }   // tools/gmap_timing.py: largest cloud alego_voxel_grid gives to one workgroup
  else if (s == "ALEGO_LOC_CHUNK") return lm_host_set_loc_chunk(h->lm, value);   // tests / tools: frames per chunk of alego_loc_enable_from_map / _update_from_map (set on the localising handle)
  else if (s == "ALEGO_PG_BUDGET") graph_ctx_set_budget(&h->pg, value);   // tests / tools: bytes of scratch per chunk of alego_graph_optimize
  else if (s == "ALEGO_LC_BUDGET") loop_ctx_set_budget(&h->lc, value);   // tests / tools: raw sub-map points per chunk of alego_loop_search
  else if (s == "ALEGO_RL_BUDGET") reloc_ctx_set(&h->rl, 0, value);   // tests / tools: (query, frame) pairs per chunk of the relocalisation search
  else if (s == "ALEGO_RL_BRUTE") reloc_ctx_set(&h->rl, 1, value);    // tests / tools: evaluate every pair instead of pruning with the ring-key bound
  else if (s == "ALEGO_SHARD_SLICE") return lm_host_debug_slice(h->lm, value & 0xff, value >> 8, &h->err);   // tests: rank | world << 8 without a communicator
  else { h->err = "unknown option " + s; return ALEGO_ERR_ARG; }
  return 0;
}

// ---- loop closure ---------------------------------------------------------------------------------------------------
int alego_loop_detect(const alego_params* P, const float* keyposes6, const double* stamps, int32_t n, const double cur_xyz[3]) {
  // detectLoopClosure :771-790 (pcl::KdTreeFLANN::radiusSearch: f32 squared distances, ascending; ties by index)
  if (!P || n <= 0 || !keyposes6 || !stamps || !cur_xyz) return -1;
  const float cx = (float)cur_xyz[0], cy = (float)cur_xyz[1], cz = (float)cur_xyz[2];
  const float r2 = nn_r2(P->lc_search_radius);
  std::vector<std::pair<float, int>> cand;
  for (int i = 0; i < n; ++i) {
    const float r = nn_d2(keyposes6[i * 6 + 0], keyposes6[i * 6 + 1], keyposes6[i * 6 + 2], cx, cy, cz);
    if (nn_in_radius(r, r2)) cand.emplace_back(r, i);
  }
  std::sort(cand.begin(), cand.end());
  for (const auto& c : cand)
    if (stamps[n - 1] - stamps[c.second] > P->lc_min_time_gap) return c.second;
  return -1;
}
int alego_loop_closure_icp(alego_handle* h, const alego_kf_in* latest, const alego_kf_in* history, int32_t n_history, alego_icp_result* out,
                           alego_point* target_out, int32_t target_cap) {
  ALEGO_GATE(h);
  if (!latest || !out || n_history < 0 || (n_history > 0 && !history)) return ALEGO_ERR_ARG;
  return icp_run(h->P, latest, history, n_history, out, target_out, target_out ? target_cap : 0, h->stream, &h->err);
}

int alego_loop_search(alego_handle* h, const int32_t* slots, int32_t n, alego_loop_result* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_loop_search", ARCHIVE)) return r;
  if (int r = gate_slot_list("alego_loop_search", slots, n, h->d.n_slots, false, &h->err)) return r;
  WAIT_ALL(h);
  return loop_search(&h->lc, *lm_host_ctx(h->lm), h->P, h->d.n_slots, slots, n, out, h->stream, &h->err);
}
// :714-730 on the host: t_correct = correction * initial_guess (Matrix4f), r_correct = Quaternionf(t_correct rotation), pose_from =
// Pose3(Rot3::Quaternion(r_correct), t_correct translation), pose_to = Pose3(Rot3::RzRyRx(closest roll, pitch, yaw), closest xyz),
// between = pose_from^-1 * pose_to.  initial_guess's rotation is AngleAxisf(yaw, Z) * AngleAxisf(pitch, Y) * AngleAxisf(roll, X) (:680-687).
int alego_loop_constraint(const float correction[16], const float latest_pose6[6], const float closest_pose6[6], float t_correct[16], double between12[12]) {
  if (!correction || !latest_pose6 || !closest_pose6 || !t_correct || !between12) return ALEGO_ERR_ARG;
  const float* kp = latest_pose6;
  const float hz = 0.5f * kp[5], hy = 0.5f * kp[4], hx = 0.5f * kp[3];
  const float qz[4] = {std::cos(hz), 0.f, 0.f, std::sin(hz)}, qy[4] = {std::cos(hy), 0.f, std::sin(hy), 0.f}, qx[4] = {std::cos(hx), std::sin(hx), 0.f, 0.f};
  float t[4], q[4];
  t[0] = qz[0] * qy[0] - qz[1] * qy[1] - qz[2] * qy[2] - qz[3] * qy[3];
  t[1] = qz[0] * qy[1] + qz[1] * qy[0] + qz[2] * qy[3] - qz[3] * qy[2];
  t[2] = qz[0] * qy[2] + qz[2] * qy[0] + qz[3] * qy[1] - qz[1] * qy[3];
  t[3] = qz[0] * qy[3] + qz[3] * qy[0] + qz[1] * qy[2] - qz[2] * qy[1];
  q[0] = t[0] * qx[0] - t[1] * qx[1] - t[2] * qx[2] - t[3] * qx[3];
  q[1] = t[0] * qx[1] + t[1] * qx[0] + t[2] * qx[3] - t[3] * qx[2];
  q[2] = t[0] * qx[2] + t[2] * qx[0] + t[3] * qx[1] - t[1] * qx[3];
  q[3] = t[0] * qx[3] + t[3] * qx[0] + t[1] * qx[2] - t[2] * qx[1];
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const float G[16] = {1 - (tyy + tzz), txy - twz, txz + twy, kp[0], txy + twz, 1 - (txx + tzz), tyz - twx, kp[1],
                       txz - twy, tyz + twx, 1 - (txx + tyy), kp[2], 0.f, 0.f, 0.f, 1.f};
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      float acc = 0.f;
      for (int k = 0; k < 4; ++k) acc += correction[r * 4 + k] * G[k * 4 + c];
      t_correct[r * 4 + c] = acc;
    }
  // Eigen's Quaternionf(Matrix3f): trace branch or largest-diagonal branch, f32
  const float* M = t_correct;
  float qf[4];   // w, x, y, z
  float tr = M[0] + M[5] + M[10];
  if (tr > 0.f) {
    tr = std::sqrt(tr + 1.f); qf[0] = 0.5f * tr; tr = 0.5f / tr;
    qf[1] = (M[9] - M[6]) * tr; qf[2] = (M[2] - M[8]) * tr; qf[3] = (M[4] - M[1]) * tr;
  } else {
    int i = 0;
    if (M[5] > M[0]) i = 1;
    if (M[10] > M[i * 5]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    tr = std::sqrt(M[i * 5] - M[j * 5] - M[k * 5] + 1.f);
    qf[1 + i] = 0.5f * tr; tr = 0.5f / tr;
    qf[0] = (M[k * 4 + j] - M[j * 4 + k]) * tr; qf[1 + j] = (M[j * 4 + i] + M[i * 4 + j]) * tr; qf[1 + k] = (M[k * 4 + i] + M[i * 4 + k]) * tr;
  }
  // Rot3::Quaternion(w, x, y, z) = Eigen::Quaterniond(...).toRotationMatrix() (f64)
  const double qw = qf[0], qxd = qf[1], qyd = qf[2], qzd = qf[3];
  const double dx = 2 * qxd, dy = 2 * qyd, dz = 2 * qzd;
  const double dwx = dx * qw, dwy = dy * qw, dwz = dz * qw, dxx = dx * qxd, dxy = dy * qxd, dxz = dz * qxd, dyy = dy * qyd, dyz = dz * qyd, dzz = dz * qzd;
  const double Rf[9] = {1 - (dyy + dzz), dxy - dwz, dxz + dwy, dxy + dwz, 1 - (dxx + dzz), dyz - dwx, dxz - dwy, dyz + dwx, 1 - (dxx + dyy)};
  const double tf[3] = {M[3], M[7], M[11]};
  // Rot3::RzRyRx(roll, pitch, yaw) (f64)
  const double cx = std::cos((double)closest_pose6[3]), sx = std::sin((double)closest_pose6[3]);
  const double cy = std::cos((double)closest_pose6[4]), sy = std::sin((double)closest_pose6[4]);
  const double cz = std::cos((double)closest_pose6[5]), sz = std::sin((double)closest_pose6[5]);
  const double ss_ = sx * sy, cs_ = cx * sy, sc_ = sx * cy, cc_ = cx * cy, c_s = cx * sz, s_s = sx * sz, _cs = cy * sz, _cc = cy * cz, s_c = sx * cz, c_c = cx * cz;
  const double ssc = ss_ * cz, csc = cs_ * cz, sss = ss_ * sz, css = cs_ * sz;
  const double Rt[9] = {_cc, -c_s + ssc, s_s + csc, _cs, c_c + sss, -s_c + css, -sy, sc_, cc_};
  const double tt[3] = {closest_pose6[0], closest_pose6[1], closest_pose6[2]};
  // Pose3::between: R = Rf^T Rt, t = Rf^T (tt - tf)
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) between12[r * 4 + c] = Rf[0 * 3 + r] * Rt[0 * 3 + c] + Rf[1 * 3 + r] * Rt[1 * 3 + c] + Rf[2 * 3 + r] * Rt[2 * 3 + c];
    between12[r * 4 + 3] = Rf[0 * 3 + r] * (tt[0] - tf[0]) + Rf[1 * 3 + r] * (tt[1] - tf[1]) + Rf[2 * 3 + r] * (tt[2] - tf[2]);
  }
  return ALEGO_OK;
}
int alego_debug_nn1(alego_handle* h, const alego_point* tgt, int32_t n_tgt, const alego_point* queries, int32_t n_q, int32_t* idx, float* d2) {
  ALEGO_GATE(h);
  if (n_tgt < 0 || n_q < 0 || (n_tgt > 0 && !tgt) || (n_q > 0 && (!queries || !idx || !d2))) return ALEGO_ERR_ARG;
  return loop_debug_nn1(tgt, n_tgt, queries, n_q, idx, d2, h->stream, &h->err);
}

// ---- the key-pose graph -----------------------------------------------------------------------------------------------
int alego_graph_enable(alego_handle* h, int32_t max_loops, const double odom_variance[6]) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_graph_enable", ARCHIVE_FIRST)) return r;
  if (h->graph_on) { h->err = "alego_graph_enable: already enabled"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  if (int r = lm_host_graph_enable(h->lm, max_loops, odom_variance, &h->err)) return r;
  h->graph_on = true;
  return 0;
}
int alego_graph_status(alego_handle* h, int slot, int32_t out[4]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!out) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_graph_status", GRAPH)) return r;
  if (int r = DevTry(__func__, &h->err).wait(stream_of(h, slot))) return r;
  return graph_status(*lm_host_ctx(h->lm), slot, out, &h->err);
}
int alego_graph_get_edges(alego_handle* h, int slot, int kind, int32_t first, int32_t n, alego_graph_edge* out) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = gate_need(h, "alego_graph_get_edges", GRAPH)) return r;
  if (int r = DevTry(__func__, &h->err).wait(stream_of(h, slot))) return r;
  return graph_get_edges(*lm_host_ctx(h->lm), slot, kind, first, n, out, &h->err);
}
int alego_graph_set_edges(alego_handle* h, int slot, int32_t first, int32_t n, const alego_graph_edge* chain) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = gate_need(h, "alego_graph_set_edges", GRAPH)) return r;
  if (int r = DevTry(__func__, &h->err).wait(stream_of(h, slot))) return r;
  return graph_set_edges(*lm_host_ctx(h->lm), slot, first, n, chain, &h->err);
}
int alego_graph_add_loops(alego_handle* h, const int32_t* slots, int32_t n, const alego_loop_result* r) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !r))) return ALEGO_ERR_ARG;
  if (int rc = gate_need(h, "alego_graph_add_loops", GRAPH)) return rc;
  if (int rc = gate_slot_list("alego_graph_add_loops", slots, n, h->d.n_slots, false, &h->err)) return rc;
  std::vector<PgAppend> a;
  for (int i = 0; i < n; ++i) {
    if (r[i].status != 2) continue;
    PgAppend p;
    std::memset(&p, 0, sizeof(p));
    p.slot = slots[i];
    p.e.from = r[i].latest_id; p.e.to = r[i].closest_id;
    std::memcpy(p.e.between, r[i].between, sizeof(p.e.between));
    for (int k = 0; k < 6; ++k) p.e.variance[k] = r[i].noise_variance;
    std::memcpy(p.corr, r[i].correction, sizeof(p.corr));
    a.push_back(p);
  }
  WAIT_ALL(h);
  return graph_append(&h->pg, *lm_host_ctx(h->lm), h->d.n_slots, a, h->stream, &h->err);
}
int alego_graph_add_edge(alego_handle* h, int slot, const alego_graph_edge* e, const float correction[16]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!e) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_graph_add_edge", GRAPH)) return r;
  PgAppend p;
  std::memset(&p, 0, sizeof(p));
  p.slot = slot; p.e = *e;
  for (int k = 0; k < 16; ++k) p.corr[k] = correction ? correction[k] : (k % 5 == 0 ? 1.f : 0.f);
  WAIT_ALL(h);
  return graph_append(&h->pg, *lm_host_ctx(h->lm), h->d.n_slots, std::vector<PgAppend>(1, p), h->stream, &h->err);
}
int alego_graph_optimize(alego_handle* h, const int32_t* slots, int32_t n, const alego_graph_opts* opts, alego_graph_result* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_graph_optimize", GRAPH)) return r;
  if (int r = gate_slot_list("alego_graph_optimize", slots, n, h->d.n_slots, true, &h->err)) return r;
  alego_graph_opts o = {ALEGO_GRAPH_MAX_ITERS, ALEGO_GRAPH_STEP_TOL, 0};
  if (opts) { if (opts->max_iters > 0) o.max_iters = opts->max_iters; if (opts->step_tol > 0.0) o.step_tol = opts->step_tol; o.apply = opts->apply != 0; }
  if (n == 0) return 0;
  WAIT_ALL(h);
  std::vector<int> apply;
  if (int r = graph_optimize(&h->pg, *lm_host_ctx(h->lm), h->d.n_slots, slots, n, o, out, &apply, h->stream, &h->err)) return r;
  int most = 0;
  for (int i = 0; i < n; ++i) if (out[i].applied) most = std::max(most, out[i].n_poses);
  if (most == 0) return 0;
  const int* apply_dev = nullptr;
  if (int r = graph_upload_apply(h->pg, apply, &apply_dev, h->stream, &h->err)) return r;
  return lm_host_graph_apply(h->lm, apply, apply_dev, most, &h->err);
}
int alego_graph_get_estimate(alego_handle* h, int slot, int32_t first, int32_t n, double* poses12) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = gate_need(h, "alego_graph_get_estimate", GRAPH)) return r;
  return graph_get_estimate(*lm_host_ctx(h->lm), slot, first, n, poses12, &h->err);
}
int alego_graph_residuals(const double* poses12, int32_t n_poses, const alego_graph_edge* edges, int32_t n_edges, double* whitened6, double* jac_from36, double* jac_to36) {
  if (!poses12 || n_poses <= 0 || n_edges < 0 || (n_edges > 0 && !edges)) return ALEGO_ERR_ARG;
  for (long i = 0; i < (long)n_poses * 12; ++i) if (!std::isfinite(poses12[i])) return ALEGO_ERR_ARG;
  return graph_residuals_host(poses12, n_poses, edges, n_edges, whitened6, jac_from36, jac_to36);
}
// marginal covariances and the loop-edge gate: nothing of a slot changes
int alego_graph_marginals(alego_handle* h, const int32_t* slots, int32_t n, int32_t cap, double* cov36, alego_graph_cov_result* out) {
  ALEGO_GATE(h);
  if (n < 0 || cap <= 0 || (n > 0 && (!slots || !cov36 || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_graph_marginals", GRAPH)) return r;
  if (int r = gate_slot_list("alego_graph_marginals", slots, n, h->d.n_slots, true, &h->err)) return r;
  if (n == 0) return 0;
  WAIT_ALL(h);
  return graph_marginals(&h->pg, *lm_host_ctx(h->lm), h->d.n_slots, slots, n, cap, cov36, out, h->stream, &h->err);
}
static int graph_check_common(alego_handle* h, const char* what, const int32_t* slots, int32_t n, const alego_graph_edge* e, const char* active, alego_graph_check* out) {
  if (int r = gate_slot_list(what, slots, n, h->d.n_slots, false, &h->err)) return r;
  if (n == 0) return 0;
  WAIT_ALL(h);
  return graph_check(&h->pg, *lm_host_ctx(h->lm), h->d.n_slots, slots, n, e, active, out, h->stream, &h->err);
}
int alego_graph_check_edges(alego_handle* h, const int32_t* slots, int32_t n, const alego_graph_edge* e, alego_graph_check* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !e || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_graph_check_edges", GRAPH)) return r;
  return graph_check_common(h, "alego_graph_check_edges", slots, n, e, nullptr, out);
}
int alego_graph_check_loops(alego_handle* h, const int32_t* slots, int32_t n, const alego_loop_result* r, alego_graph_check* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !r || !out))) return ALEGO_ERR_ARG;
  if (int rc = gate_need(h, "alego_graph_check_loops", GRAPH)) return rc;
  std::vector<alego_graph_edge> e(std::max(n, 1));
  std::vector<char> active(std::max(n, 1), 0);
  for (int i = 0; i < n; ++i) {
    std::memset(&e[i], 0, sizeof(e[i]));
    if (r[i].status != 2) continue;
    active[i] = 1;
    e[i].from = r[i].latest_id; e[i].to = r[i].closest_id;
    std::memcpy(e[i].between, r[i].between, sizeof(e[i].between));
    for (int k = 0; k < 6; ++k) e[i].variance[k] = r[i].noise_variance;
  }
  return graph_check_common(h, "alego_graph_check_loops", slots, n, e.data(), active.data(), out);
}
int alego_graph_covariance_host(const double* poses12, int32_t n_poses, const alego_graph_edge* edges, int32_t n_edges, const int32_t* pairs, int32_t n_pairs,
                                double* marg36, double* pair36) {
  return graph_covariance_host(poses12, n_poses, edges, n_edges, pairs, n_pairs, marg36, pair36);
}
int alego_graph_check_host(const double* poses12, int32_t n_poses, const alego_graph_edge* edges, int32_t n_edges, const alego_graph_edge* cand, int32_t n_cand,
                           alego_graph_check* out) {
  return graph_check_host(poses12, n_poses, edges, n_edges, cand, n_cand, out);
}

// ---- covariance and degeneracy of the scan-to-map registration --------------------------------
int alego_regcov_enable(alego_handle* h, const alego_regcov_opts* opts) {
  ALEGO_GATE(h);
  if (!h->lm) { h->err = "alego_regcov_enable: the handle has no LaserMapping"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  return lm_host_regcov_enable(h->lm, opts, &h->err);
}
int alego_regcov_get(alego_handle* h, const int32_t* slots, int32_t n, alego_regcov* out) {
  ALEGO_GATE(h);
  if (!h->lm || n < 0 || (n > 0 && (!slots || !out))) { h->err = "alego_regcov_get: null argument / negative count"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  return lm_host_regcov_get(h->lm, slots, n, out, &h->err);
}
int alego_regcov_host(const double acc28[28], const double params6[6], int32_t n_edge, int32_t n_plane, const alego_regcov_opts* opts, alego_regcov* out) {
  if (!acc28 || !params6 || !out || n_edge < 0 || n_plane < 0) return ALEGO_ERR_ARG;
  double dflt[RC_OPT_W], opt[RC_OPT_W];
  (void)lm_host_regcov_opts(nullptr, dflt);
  if (rc_resolve(opts ? &opts->sigma0 : nullptr, dflt + RC_VAR_MIN, opt)) return ALEGO_ERR_ARG;
  regcov_host(acc28, params6, n_edge, n_plane, opt, out);
  return 0;
}
int alego_regcov_normal_host(const double params6[6], const double* edge_rows9, int32_t n_edge, const double* plane_rows7, int32_t n_plane, double huber, double acc28[28]) {
  if (!params6 || !acc28 || n_edge < 0 || n_plane < 0 || (n_edge > 0 && !edge_rows9) || (n_plane > 0 && !plane_rows7)) return ALEGO_ERR_ARG;
  regcov_normal_host(params6, edge_rows9, n_edge, plane_rows7, n_plane, huber, acc28);
  return 0;
}
// Caller rows as lm_fit leaves a slot (lm_rows.h), for the two debug entries below: block records of the edges from row 0 and of the planes from
// row nqc (nqc >= n_edge corner queries, those past n_edge without a row), and the query points as f32; no vector is empty.
static void stage_caller_rows(const double* edge_rows9, int n_edge, const double* plane_rows7, int n_plane, int nqc, std::vector<double>* blocks, std::vector<float>* qc,
                              std::vector<float>* qs) {
  const size_t nqs = (size_t)std::max(n_plane, 1);
  blocks->assign(((size_t)nqc + nqs) * LMB_W, 0.0);
  qc->assign(std::max<size_t>((size_t)nqc, 1) * 4, 0.f);
  qs->assign(nqs * 4, 0.f);
  for (int i = 0; i < n_edge; ++i) {
    const double* r = edge_rows9 + (size_t)i * 9;
    lmb_put_edge(&(*blocks)[lm_row_of(0, i, nqc) * LMB_W], r, r + 3);
    for (int k = 0; k < 3; ++k) (*qc)[(size_t)i * 4 + k] = (float)r[6 + k];
  }
  for (int i = 0; i < n_plane; ++i) {
    const double* r = plane_rows7 + (size_t)i * 7;
    lmb_put_plane(&(*blocks)[lm_row_of(1, i, nqc) * LMB_W], r, r[3]);
    for (int k = 0; k < 3; ++k) (*qs)[(size_t)i * 4 + k] = (float)r[4 + k];
  }
}
int alego_debug_regcov(alego_handle* h, const double params6[6], const double* edge_rows9, int32_t n_edge, const double* plane_rows7, int32_t n_plane, alego_regcov* out) {
  ALEGO_GATE(h);
  if (!params6 || !out || n_edge < 0 || n_plane < 0 || (n_edge > 0 && !edge_rows9) || (n_plane > 0 && !plane_rows7)) { h->err = "alego_debug_regcov: null argument / negative count"; return ALEGO_ERR_ARG; }
  double opt[RC_OPT_W];
  (void)lm_host_regcov_opts(h->lm, opt);
  std::vector<double> blocks;
  std::vector<float> qc, qs;
  stage_caller_rows(edge_rows9, n_edge, plane_rows7, n_plane, n_edge, &blocks, &qc, &qs);
  DevPool T;   // temporaries of this call
  double *db, *dp, *dopt;
  float4 *dqc, *dqs;
  alego_regcov* drec;
  HIP_TRY(h, T.get(&db, blocks.size(), false)); HIP_TRY(h, T.get(&dp, 6, false)); HIP_TRY(h, T.get(&dopt, (size_t)RC_OPT_W, false));
  HIP_TRY(h, T.get(&dqc, qc.size() / 4, false)); HIP_TRY(h, T.get(&dqs, qs.size() / 4, false)); HIP_TRY(h, T.get(&drec, 1, true));
  DevTry c(__func__, &h->err);
  if (c.up(db, blocks).up(dp, params6, 6).up(dopt, opt).up(reinterpret_cast<float*>(dqc), qc).up(reinterpret_cast<float*>(dqs), qs)) return c;   // (the queries are staged as floats, four to a point)
  launch_lm_regcov_debug(db, dqc, n_edge, dqs, n_plane, dp, h->d.P.huber_delta, dopt, drec, h->stream);
  return c.wait(h->stream).down(out, drec, 1);
}

// ---- solution remapping of the scan-to-map registration ----------------------------------------
int alego_remap_enable(alego_handle* h, const alego_remap_opts* opts) {
  ALEGO_GATE(h);
  if (!h->lm) { h->err = "alego_remap_enable: the handle has no LaserMapping"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  return lm_host_remap_enable(h->lm, opts, &h->err);
}
int alego_remap_get(alego_handle* h, const int32_t* slots, int32_t n, alego_remap* out) {
  ALEGO_GATE(h);
  if (!h->lm || n < 0 || (n > 0 && (!slots || !out))) { h->err = "alego_remap_get: null argument / negative count"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  return lm_host_remap_get(h->lm, slots, n, out, &h->err);
}
int alego_remap_host(const double acc28[28], const double params6[6], int32_t n_edge, int32_t n_plane, const alego_remap_opts* opts, alego_remap* out) {
  if (!acc28 || !params6 || !out || n_edge < 0 || n_plane < 0) return ALEGO_ERR_ARG;
  double eig_min;
  if (rm_resolve(opts ? &opts->eig_min : nullptr, &eig_min)) return ALEGO_ERR_ARG;
  remap_host(acc28, params6, n_edge, n_plane, eig_min, out);
  return 0;
}
int alego_remap_step_host(const double H21[21], const double g6[6], const double scale6[6], double radius, const double* proj36, double step6[6], double* mcc) {
  if (!H21 || !g6 || !scale6 || !step6 || !mcc) return ALEGO_ERR_ARG;
  return remap_step_host(H21, g6, scale6, radius, proj36, step6, mcc) == LM_EVAL ? 1 : 0;
}
int alego_debug_remap_solve(alego_handle* h, const double start6[6], const double* edge_rows9, int32_t n_edge, const double* plane_rows7, int32_t n_plane, int32_t remap,
                            double* params_it, double* costs, int32_t* summary, alego_remap* rec) {
  ALEGO_GATE(h);
  if (!h->lm) { h->err = "alego_debug_remap_solve: the handle has no LaserMapping"; return ALEGO_ERR_ARG; }
  if (!start6 || !params_it || !costs || !summary || n_edge < 0 || n_plane < 0 || (n_edge > 0 && !edge_rows9) || (n_plane > 0 && !plane_rows7)) {
    h->err = "alego_debug_remap_solve: null argument / negative count"; return ALEGO_ERR_ARG;
  }
  // one slot as lm_fit leaves it (lm_rows.h): the corner queries padded with queries that gave no row up to the registration guard's minimum, the
  // planes' block records from row nqc, the query points as f32; the guard's other counts at values that pass it
  const alego_params& P = h->d.P;
  const int nqc = std::max({(int)n_edge, P.lm_min_corner, 1}), nqs = n_plane;
  const size_t nr = (size_t)nqc + (size_t)std::max(nqs, 1);
  std::vector<double> blocks, ld(LD_COUNT, 0.0);
  std::vector<float> qc, qs;
  std::vector<int> li(LI_COUNT, 0);
  stage_caller_rows(edge_rows9, n_edge, plane_rows7, n_plane, nqc, &blocks, &qc, &qs);
  li[LI_RUN] = 1; li[LI_NKF] = 1; li[LI_REC_CNT] = 1; li[LI_NCUR_C] = nqc; li[LI_NTOTAL_DS] = nqs;
  li[LI_NTOTAL] = std::max(nqs, P.lm_min_surf); li[LI_KDS_C] = std::max(1, P.lm_min_map_corner);
  for (int k = 0; k < 6; ++k) ld[LD_PARAMS + k] = start6[k];
  DevPool T;   // temporaries of this call
  LmCtx L;
  std::memset(&L, 0, sizeof L);
  L.kf_cap_c = nqc; L.total_cap = std::max(nqs, 1); L.qcap = (int)nr;
  L.solve_row_bytes = lm_host_ctx(h->lm)->solve_row_bytes;
  L.rm_eig_min = lm_host_remap_eig_min(h->lm);
  HIP_TRY(h, T.get(&L.li, li.size(), false)); HIP_TRY(h, T.get(&L.ld, ld.size(), false)); HIP_TRY(h, T.get(&L.blocks, blocks.size(), false));
  HIP_TRY(h, T.get(&L.crows, nr * LMS_W, true)); HIP_TRY(h, T.get(&L.cur_corner_ds, qc.size() / 4, false)); HIP_TRY(h, T.get(&L.cur_total_ds, qs.size() / 4, false));
  HIP_TRY(h, T.get(&L.rm_rec, 1, true));
  DevTry c(__func__, &h->err);
  if (c.up(L.li, li).up(L.ld, ld).up(L.blocks, blocks).up(reinterpret_cast<float*>(L.cur_corner_ds), qc).up(reinterpret_cast<float*>(L.cur_total_ds), qs)) return c;
  DevCtx d = h->d;
  d.slot0 = 0; d.n_launch = 1;
  launch_lm_solve(d, L, remap != 0, h->stream);
  if (c.wait(h->stream).down(li, L.li).down(ld, L.ld)) return c;
  for (int k = 0; k < 12; ++k) params_it[k] = ld[LD_PARAMS_IT + k];
  for (int k = 0; k < 4; ++k) costs[k] = ld[LD_COSTS + k];
  summary[0] = li[LI_SUM0]; summary[1] = li[LI_SUM1];
  if (rec) c.down(rec, L.rm_rec, 1);
  return c;
}

// ---- one registration sharded over the GPUs of a node ---------------------------------------------------------------
int alego_dist_unique_id(char id[ALEGO_DIST_ID_BYTES]) { return id ? lm_host_dist_unique_id(id) : ALEGO_ERR_ARG; }
int alego_dist_init(alego_handle* h, int rank, int world, const char id[ALEGO_DIST_ID_BYTES]) {
  ALEGO_GATE(h);
  if (!id) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_dist_init", MAPPING)) return r;
  drain_back(h);
  return lm_host_dist_init(h->lm, rank, world, id, &h->err);
}
int alego_dist_allreduce_probe(alego_handle* h, int iters, double* usec_per_allreduce) {
  ALEGO_GATE(h);
  drain_back(h);
  return lm_host_dist_probe(h->lm, iters, usec_per_allreduce, &h->err);
}
int alego_dist_shutdown(alego_handle* h) {
  ALEGO_GATE(h);
  drain_back(h);
  return lm_host_dist_shutdown(h->lm);
}

// ---- localisation against a frozen key-frame map (kernels_loc.hip) ---------------------------
int alego_loc_enable(alego_handle* h, const alego_kf_in* frames, int32_t n, double radius) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_loc_enable", NOT_STREAM_MODE | UNUSED_HANDLE)) return r;
  WAIT_ALL(h);
  return lm_host_loc_enable(h->lm, h->d, frames, n, radius, &h->err);
}
// ... the store built on the device from a slot's archive of a mapping handle of the same process
static int handover_source(alego_handle* h, alego_handle* map, int slot, const char* what) {
  const std::string w(what);
  if (!map) { h->err = w + ": the mapping handle is null"; return ALEGO_ERR_ARG; }
  if (map == h) { h->err = w + ": the mapping handle and the localising handle are the same"; return ALEGO_ERR_ARG; }
  if (!map->map_on) { h->err = w + ": the mapping handle has no key-frame archive (alego_map_enable)"; return ALEGO_ERR_ARG; }
  if (slot < 0 || slot >= map->d.n_slots) { h->err = w + ": slot out of range of the mapping handle"; return ALEGO_ERR_ARG; }
  if (map->device != h->device) { h->err = w + ": the two handles sit on different devices (" + std::to_string(map->device) + ", " + std::to_string(h->device) + ")"; return ALEGO_ERR_ARG; }
  return 0;
}
int alego_loc_enable_from_map(alego_handle* h, alego_handle* map, int slot, double radius, int32_t capacity) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_loc_enable_from_map", NOT_STREAM_MODE | UNUSED_HANDLE)) return r;
  if (int r = handover_source(h, map, slot, "alego_loc_enable_from_map")) return r;
  if (int r = DevTry(__func__, &h->err).wait(all_streams(map))) return r;   // a key frame still queued by alego_batch_run(.., sync = 0) is part of the hand-over
  WAIT_ALL(h);
  return lm_host_loc_enable_from_map(h->lm, h->d, map->lm, slot, radius, capacity, &h->err);
}
int alego_loc_update_from_map(alego_handle* h, alego_handle* map, int slot) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_loc_update_from_map", LOCALISING)) return r;
  if (int r = handover_source(h, map, slot, "alego_loc_update_from_map")) return r;
  if (int r = DevTry(__func__, &h->err).wait(all_streams(map))) return r;
  WAIT_ALL(h);   // behind the work queued on every stream group, front and back
  bool rewritten = false;
  const int rc = lm_host_loc_update_from_map(h->lm, map->lm, slot, &rewritten, &h->err);
  if (!rewritten) return rc;   // refused before anything was written
  std::string rerr;
  const int rr = reloc_refresh(h->rl, *lm_host_ctx(h->lm), h->stream, &rerr);
  if (rc) return rc;
  if (rr) h->err = rerr;
  return rr;
}
// ---- relocalisation (kernels_reloc.hip) ----
int alego_reloc_enable(alego_handle* h, double max_range, double z_offset) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_reloc_enable", LOCALISING_SEED)) return r;
  if (reloc_enabled(h->rl)) { h->err = "alego_reloc_enable: already enabled"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  return reloc_enable(&h->rl, *lm_host_ctx(h->lm), h->d.n_slots, max_range, z_offset, h->stream, &h->err);
}
int alego_loc_relocalize(alego_handle* h, const int32_t* slots, int32_t n, const alego_reloc_opts* opts, alego_reloc_result* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_loc_relocalize", RELOCALISATION)) return r;
  int n_cand = 4, verify = 1, apply = 0;
  if (opts) { if (opts->n_cand > 0) n_cand = opts->n_cand; if (opts->verify >= 0) verify = opts->verify; apply = opts->apply != 0; }
  if (n_cand > ALEGO_RELOC_MAX_CAND || verify > n_cand) { h->err = "alego_loc_relocalize: n_cand is 1 .. ALEGO_RELOC_MAX_CAND, verify 0 .. n_cand"; return ALEGO_ERR_ARG; }
  if (int r = gate_slot_list("alego_loc_relocalize", slots, n, h->d.n_slots, true, &h->err)) return r;
  WAIT_ALL(h);
  return reloc_run(h->rl, &h->lc, *lm_host_ctx(h->lm), h->P, slots, n, n_cand, verify, apply, out, h->stream, &h->err);
}
int alego_debug_reloc_search(alego_handle* h, const uint8_t* map_desc, int32_t n_map, const uint8_t* q_desc, int32_t n_q, int32_t n_cand,
                             int32_t* ids, int32_t* dists, int32_t* shifts) {
  ALEGO_GATE(h);
  if (n_map < 0 || n_map > (1 << 24) - 1 || n_q < 0 || n_cand < 1 || n_cand > ALEGO_RELOC_MAX_CAND || (n_map > 0 && !map_desc) || (n_q > 0 && (!q_desc || !ids || !dists || !shifts)))
    return ALEGO_ERR_ARG;
  return reloc_debug_search(&h->rl, map_desc, n_map, q_desc, n_q, n_cand, ids, dists, shifts, h->stream, &h->err);
}

// ---- loop closures by appearance (kernels_reloc.hip) ----
int alego_loop_appearance_enable(alego_handle* h, double max_range, double z_offset) {
  ALEGO_GATE(h);
  if (int r = gate_need(h, "alego_loop_appearance_enable", MAPPING | ARCHIVE_FIRST)) return r;
  if (loop_app_enabled(h->rl)) { h->err = "alego_loop_appearance_enable: already enabled"; return ALEGO_ERR_ARG; }
  return loop_app_enable(&h->rl, *lm_host_ctx(h->lm), h->d.n_slots, max_range, z_offset, &h->err);
}
int alego_loop_search_appearance(alego_handle* h, const int32_t* slots, int32_t n, const alego_loop_app_opts* opts, alego_loop_result* out, alego_loop_app_info* info) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_loop_search_appearance", APPEARANCE)) return r;
  alego_loop_app_opts o = {4, 1, 0, 0.0, 0.0};
  if (opts) { if (opts->n_cand > 0) o.n_cand = opts->n_cand; if (opts->verify >= 0) o.verify = opts->verify; o.max_dist = opts->max_dist; o.max_jump = opts->max_jump; o.fitness_max = opts->fitness_max; }
  if (o.n_cand > ALEGO_RELOC_MAX_CAND || o.verify > o.n_cand) { h->err = "alego_loop_search_appearance: n_cand is 1 .. ALEGO_RELOC_MAX_CAND, verify 0 .. n_cand"; return ALEGO_ERR_ARG; }
  if (int r = gate_slot_list("alego_loop_search_appearance", slots, n, h->d.n_slots, true, &h->err)) return r;
  WAIT_ALL(h);
  return loop_app_run(h->rl, &h->lc, *lm_host_ctx(h->lm), h->P, slots, n, o, out, info, h->stream, &h->err);
}

// ---- aligning one slot's archive to another's (kernels_reloc.hip) ----
int alego_map_align(alego_handle* h, const int32_t* src_slots, const int32_t* dst_slots, int32_t n, const alego_map_align_opts* opts, alego_map_align_result* out,
                    alego_map_align_hyp* hyp) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!src_slots || !dst_slots || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_map_align", MAPPING | APPEARANCE)) return r;
  alego_map_align_opts o;
  std::memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if (o.n_queries <= 0) o.n_queries = 8;
  if (o.n_cand <= 0) o.n_cand = 2;
  if (o.n_queries > ALEGO_ALIGN_MAX_QUERIES || o.n_cand > ALEGO_RELOC_MAX_CAND) { h->err = "alego_map_align: n_queries is 1 .. ALEGO_ALIGN_MAX_QUERIES, n_cand 1 .. ALEGO_RELOC_MAX_CAND"; return ALEGO_ERR_ARG; }
  if (int r = gate_pair_list("alego_map_align", src_slots, dst_slots, n, h->d.n_slots, GATE_PAIRS_ALIGN, &h->err)) return r;
  WAIT_ALL(h);
  return map_align_run(h->rl, &h->lc, *lm_host_ctx(h->lm), h->P, src_slots, dst_slots, n, o, out, hyp, h->stream, &h->err);
}

// ---- a slot moved, one archive appended to another's (kernels_merge.hip) ----
int alego_map_move(alego_handle* h, const int32_t* slots, int32_t n, const double* T12, int32_t* out_status) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !T12 || !out_status))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_map_move", MAPPING | ARCHIVE)) return r;
  for (int i = 0; i < n; ++i) if (!mg_finite12(T12 + (size_t)i * 12)) { h->err = "alego_map_move: a transform is not finite"; return ALEGO_ERR_ARG; }
  if (int r = gate_slot_list("alego_map_move", slots, n, h->d.n_slots, true, &h->err)) return r;
  if (n == 0) return 0;
  WAIT_ALL(h);
  return lm_host_map_move(h->lm, slots, n, T12, out_status, &h->err);
}
int alego_map_merge(alego_handle* h, const int32_t* src_slots, const int32_t* dst_slots, int32_t n, const double* T12, const alego_map_merge_opts* opts,
                    const alego_map_align_hyp* hyp, alego_map_merge_result* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!src_slots || !dst_slots || !T12 || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_map_merge", MAPPING | ARCHIVE)) return r;
  const double off = opts ? opts->stamp_offset : 0.0;
  const double* sv = opts ? opts->seam_variance : nullptr;
  if (!(off - off == 0.0)) { h->err = "alego_map_merge: stamp_offset is not finite"; return ALEGO_ERR_ARG; }
  for (int k = 0; sv && k < 6; ++k) if (!(sv[k] > 0.0) || !(sv[k] - sv[k] == 0.0)) { h->err = "alego_map_merge: seam_variance must be positive and finite"; return ALEGO_ERR_ARG; }
  for (int i = 0; i < n; ++i) if (!mg_finite12(T12 + (size_t)i * 12)) { h->err = "alego_map_merge: a transform is not finite"; return ALEGO_ERR_ARG; }
  if (int r = gate_pair_list("alego_map_merge", src_slots, dst_slots, n, h->d.n_slots, GATE_PAIRS_MERGE, &h->err)) return r;
  if (n == 0) return 0;
  WAIT_ALL(h);
  return lm_host_map_merge(h->lm, &h->pg, src_slots, dst_slots, n, T12, off, sv, hyp, out, &h->err);
}
int alego_map_align_edge(const alego_map_align_hyp* hyp, const float dst_pose6[6], int32_t nd, alego_graph_edge* edge) {
  if (!hyp || !dst_pose6 || !edge || nd < 0 || !(hyp->accepted && hyp->inlier)) return ALEGO_ERR_ARG;
  float t_correct[16];
  edge->from = nd + hyp->src_frame; edge->to = hyp->dst_frame;
  if (int r = alego_loop_constraint(hyp->icp_final, hyp->guess6, dst_pose6, t_correct, edge->between)) return r;
  for (int k = 0; k < 6; ++k) edge->variance[k] = (double)(float)hyp->fitness;
  return ALEGO_OK;
}
int alego_map_merge_edges(const alego_graph_edge* src_chain, int32_t ns, const alego_graph_edge* src_loops, int32_t n_loops, int32_t nd,
                          const float prev_pose6[6], const float first_pose6[6], const double seam_variance6[6],
                          alego_graph_edge* out_chain, alego_graph_edge* out_loops) {
  if (ns < 0 || n_loops < 0 || nd < 0 || (ns > 0 && (!src_chain || !out_chain || !first_pose6 || !seam_variance6)) || (ns > 0 && nd > 0 && !prev_pose6) ||
      (n_loops > 0 && (!src_loops || !out_loops))) return ALEGO_ERR_ARG;
  if (ns > 0) mg_seam_edge(nd, prev_pose6, first_pose6, seam_variance6, &out_chain[0]);
  for (int f = 1; f < ns; ++f) mg_shift_edge(&src_chain[f], nd, &out_chain[f]);
  for (int l = 0; l < n_loops; ++l) mg_shift_edge(&src_loops[l], nd, &out_loops[l]);
  return ALEGO_OK;
}

// ---- a slot's archive thinned in place (kernels_thin.hip) ----
int alego_map_thin(alego_handle* h, const int32_t* slots, int32_t n, const alego_map_thin_opts* opts, alego_map_thin_result* out) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!slots || !out))) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_map_thin", MAPPING | ARCHIVE)) return r;
  const double md = opts ? opts->min_dist : 0.0;
  if (!(md - md == 0.0)) { h->err = "alego_map_thin: min_dist is not finite"; return ALEGO_ERR_ARG; }
  if (int r = gate_slot_list("alego_map_thin", slots, n, h->d.n_slots, true, &h->err)) return r;
  if (n == 0) return 0;
  WAIT_ALL(h);
  std::vector<int> first((size_t)n, 0);
  const int rc = lm_host_map_thin(h->lm, slots, n, md, out, first.data(), &h->err);
  // the descriptors depend on the clouds only: a thinned slot keeps those below its first dropped frame (also after a failure half way)
  for (int i = 0; i < n; ++i) if (rc || out[i].status == 2) loop_app_forget(h->rl, slots[i], rc ? 0 : first[i]);
  return rc;
}
int alego_map_thin_select(const float* keyposes6, const uint8_t* protect, int32_t n, double min_dist, uint8_t* keep) {
  if (n < 0 || (n > 0 && (!keyposes6 || !keep)) || !(min_dist - min_dist == 0.0)) return ALEGO_ERR_ARG;
  return th_select_host(keyposes6, 6, protect, n, min_dist, keep);
}
int alego_map_thin_edges(const alego_graph_edge* chain, int32_t n, const alego_graph_edge* loops, int32_t n_loops, const uint8_t* keep,
                         alego_graph_edge* out_chain, alego_graph_edge* out_loops) {
  if (n < 0 || n_loops < 0 || (n > 0 && (!chain || !keep || !out_chain || !keep[0])) || (n_loops > 0 && (!loops || !out_loops))) return ALEGO_ERR_ARG;
  std::vector<int> new_id((size_t)n, -1);
  int m = 0;
  for (int i = 0; i < n; ++i) if (keep[i]) new_id[i] = m++;
  for (int l = 0; l < n_loops; ++l) {   // checked before anything is written: a loop edge's endpoints are kept
    alego_graph_edge x;
    if (!th_remap_edge(&loops[l], new_id.data(), n, &x)) return ALEGO_ERR_ARG;
  }
  for (int i = 0, prev = -1; i < n; ++i) {
    if (!keep[i]) continue;
    if (prev < 0) out_chain[0] = chain[0]; else th_compose_edge(chain, prev, i, new_id[i], &out_chain[new_id[i]]);
    prev = i;
  }
  for (int l = 0; l < n_loops; ++l) (void)th_remap_edge(&loops[l], new_id.data(), n, &out_loops[l]);
  return m;
}
int alego_debug_thin_select(alego_handle* h, const float* keyposes6, const uint8_t* protect, int32_t n, double min_dist, uint8_t* keep) {
  ALEGO_GATE(h);
  if (n < 0 || (n > 0 && (!keyposes6 || !protect || !keep)) || !(min_dist - min_dist == 0.0)) return ALEGO_ERR_ARG;
  WAIT_ALL(h);
  return lm_host_debug_thin_select(h->lm, keyposes6, protect, n, min_dist, keep, &h->err);
}

// ---- the occupancy grid of the archive (kernels_occ.hip, occ_math.h) ----
namespace {
int occ_need(alego_handle* h, const char* what) {
  if (int r = gate_need(h, what, MAPPING | ARCHIVE)) return r;
  if (!lm_host_occ_on(h->lm)) { h->err = std::string(what) + ": the occupancy grid is off (alego_occ_enable)"; return ALEGO_ERR_ARG; }
  return 0;
}
}  // namespace
int alego_occ_enable(alego_handle* h, const alego_occ_opts* opts) {
  ALEGO_GATE(h);
  if (!opts) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_occ_enable", MAPPING | ARCHIVE)) return r;
  if (lm_host_occ_on(h->lm)) { h->err = "alego_occ_enable: already enabled"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  return lm_host_occ_enable(h->lm, opts, &h->err);
}
int alego_occ_clear(alego_handle* h) {
  ALEGO_GATE(h);
  if (int r = occ_need(h, "alego_occ_clear")) return r;
  return lm_host_occ_clear(h->lm, &h->err);
}
int alego_occ_integrate(alego_handle* h, int slot, int32_t first, int32_t n, int kinds, int64_t stats[ALEGO_OCC_STATS]) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = occ_need(h, "alego_occ_integrate")) return r;
  return lm_host_occ_integrate(h->lm, slot, first, n, kinds, stats, &h->err);
}
int alego_occ_get(alego_handle* h, uint32_t* hits, uint32_t* passes) {
  ALEGO_GATE(h);
  if (int r = occ_need(h, "alego_occ_get")) return r;
  return lm_host_occ_get(h->lm, hits, passes, &h->err);
}
int alego_occ_classify(alego_handle* h, const alego_occ_rule* rule, int collapse_z, int8_t* out) {
  ALEGO_GATE(h);
  if (!out) return ALEGO_ERR_ARG;
  if (int r = occ_need(h, "alego_occ_classify")) return r;
  const alego_occ_rule dflt = {1, 2, 1, 0};
  const alego_occ_rule& R = rule ? *rule : dflt;
  if (const char* why = occ_rule_fault(&R)) { h->err = std::string("alego_occ_classify: ") + why; return ALEGO_ERR_ARG; }
  return lm_host_occ_classify(h->lm, R, collapse_z, out, &h->err);
}
int alego_debug_occ_piece(alego_handle* h, int32_t piece) {
  ALEGO_GATE(h);
  return lm_host_occ_set_piece(h->lm, piece);
}
int alego_occ_ray_host(const alego_occ_opts* opts, const float o[3], const float e[3], int32_t* cells3, int32_t cap, int32_t* hit) {
  if (!opts || !o || !e || cap < 0 || (cap > 0 && !cells3) || occ_opts_fault(opts)) return ALEGO_ERR_ARG;
  const int64_t n = occ_ray_host(occ_grid(opts), o, e, cells3, cap, hit);
  return n > 2147483647LL ? 2147483647 : (int)n;
}
int alego_occ_integrate_host(const alego_occ_opts* opts, const alego_point* origins, const alego_point* pts, int32_t n_pts, uint32_t* hits, uint32_t* passes,
                             int64_t stats[ALEGO_OCC_STATS]) {
  if (!opts || n_pts < 0 || (n_pts > 0 && (!origins || !pts)) || occ_opts_fault(opts)) return ALEGO_ERR_ARG;
  const OccGrid G = occ_grid(opts);
  for (int i = 0; i < n_pts; ++i) if (!(pts[i].intensity >= 0.f)) return ALEGO_ERR_ARG;   // (not a frame id: refused before anything is added)
  int64_t local[ALEGO_OCC_STATS] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n_pts; ++i) {
    const alego_point& kp = origins[(int)pts[i].intensity];
    const float o[3] = {kp.x, kp.y, kp.z}, e[3] = {pts[i].x, pts[i].y, pts[i].z};
    occ_add_host(G, o, e, hits, passes, local);
  }
  if (stats) for (int k = 0; k < ALEGO_OCC_STATS; ++k) stats[k] += local[k];
  return 0;
}
int alego_occ_classify_host(const alego_occ_opts* opts, const alego_occ_rule* rule, const uint32_t* hits, const uint32_t* passes, int collapse_z, int8_t* out) {
  if (!opts || !hits || !passes || !out || occ_opts_fault(opts)) return ALEGO_ERR_ARG;
  const alego_occ_rule dflt = {1, 2, 1, 0};
  const alego_occ_rule& R = rule ? *rule : dflt;
  if (occ_rule_fault(&R)) return ALEGO_ERR_ARG;
  occ_classify_host(occ_grid(opts), R, hits, passes, collapse_z, out);
  return 0;
}

// ---- the clearance field and the cost map (kernels_edt.hip, edt_math.h) ----
int alego_occ_set(alego_handle* h, const uint32_t* hits, const uint32_t* passes) {
  ALEGO_GATE(h);
  if (int r = occ_need(h, "alego_occ_set")) return r;
  return lm_host_occ_set(h->lm, hits, passes, &h->err);
}
int alego_occ_distance(alego_handle* h, const alego_occ_rule* rule, const alego_occ_dist_opts* opts, uint32_t* d2, int64_t stats[ALEGO_EDT_STATS]) {
  ALEGO_GATE(h);
  if (int r = occ_need(h, "alego_occ_distance")) return r;
  const alego_occ_rule dflt = {1, 2, 1, 0};
  const alego_occ_rule& R = rule ? *rule : dflt;
  if (const char* why = occ_rule_fault(&R)) { h->err = std::string("alego_occ_distance: ") + why; return ALEGO_ERR_ARG; }
  const alego_occ_dist_opts O = opts ? *opts : alego_occ_dist_opts{0, 0, 0, 0};
  return lm_host_occ_distance(h->lm, R, O, d2, stats, &h->err);
}
int alego_occ_costmap(alego_handle* h, const alego_occ_rule* rule, int collapse_z, int unknown_is_obstacle, const alego_occ_inflation* infl, uint8_t* out) {
  ALEGO_GATE(h);
  if (!infl || !out) return ALEGO_ERR_ARG;
  if (int r = occ_need(h, "alego_occ_costmap")) return r;
  const alego_occ_rule dflt = {1, 2, 1, 0};
  const alego_occ_rule& R = rule ? *rule : dflt;
  if (const char* why = occ_rule_fault(&R)) { h->err = std::string("alego_occ_costmap: ") + why; return ALEGO_ERR_ARG; }
  return lm_host_occ_costmap(h->lm, R, collapse_z, unknown_is_obstacle, *infl, out, &h->err);
}
int alego_occ_distance_host(const int8_t* cls, const int32_t n[3], int unknown_is_obstacle, int32_t max_cells, uint32_t* d2, int64_t stats[ALEGO_EDT_STATS]) {
  if (!cls || !n || (!d2 && !stats) || edt_dims_fault(n, max_cells)) return ALEGO_ERR_ARG;
  const size_t cells = (size_t)n[0] * n[1] * n[2];
  std::vector<uint32_t> work(cells), own(d2 ? 0 : cells);
  std::vector<EdtTop> stack((size_t)std::max(n[0], std::max(n[1], n[2])));
  edt_distance_host(cls, n, unknown_is_obstacle, max_cells, d2 ? d2 : own.data(), work.data(), stack.data(), stats);
  return 0;
}
int alego_occ_cost_table_host(double s, const alego_occ_inflation* infl, uint8_t* table, int32_t cap) {
  int32_t r = 0;
  if (!infl || cap < 0 || (cap > 0 && !table) || edt_inflation_fault(s, infl, &r)) return ALEGO_ERR_ARG;
  if (cap < r * r + 1) return ALEGO_ERR_CAPACITY;
  edt_cost_table(s, infl, r, table);
  return r * r + 1;
}
int alego_occ_costmap_host(const int8_t* cls, const uint32_t* d2, int64_t cells, int unknown_is_obstacle, const uint8_t* table, int32_t n_table, int inflate_unknown,
                           uint8_t* out) {
  if (cells < 0 || n_table < 1 || !table || (cells > 0 && (!cls || !d2 || !out))) return ALEGO_ERR_ARG;
  for (int64_t i = 0; i < cells; ++i) out[i] = edt_cost(cls[i], d2[i], unknown_is_obstacle, table, n_table, inflate_unknown);
  return 0;
}

// ---- the static map ----
int alego_occ_mark(alego_handle* h, int slot, int kinds, const alego_static_rule* rule, uint8_t* verdict, int32_t cap, int64_t stats[ALEGO_STATIC_VERDICTS]) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = occ_need(h, "alego_occ_mark")) return r;
  const alego_static_rule R = rule ? *rule : occ_static_rule_default();
  if (const char* why = occ_static_rule_fault(&R)) { h->err = std::string("alego_occ_mark: ") + why; return ALEGO_ERR_ARG; }
  return lm_host_occ_mark(h->lm, slot, kinds, R, verdict, cap, stats, &h->err);
}
int alego_map_assemble_static(alego_handle* h, int slot, int kinds, float leaf, const alego_static_rule* rule, alego_point* out, int32_t cap,
                              int64_t stats[ALEGO_STATIC_VERDICTS]) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = occ_need(h, "alego_map_assemble_static")) return r;
  const alego_static_rule R = rule ? *rule : occ_static_rule_default();
  if (const char* why = occ_static_rule_fault(&R)) { h->err = std::string("alego_map_assemble_static: ") + why; return ALEGO_ERR_ARG; }
  return lm_host_map_assemble_static(h->lm, slot, kinds, leaf, R, out, cap, stats, &h->err);
}
int alego_occ_mark_host(const alego_occ_opts* opts, const alego_static_rule* rule, const uint32_t* hits, const uint32_t* passes, const alego_point* pts,
                        const float* sensor_z, int32_t n, uint8_t* verdict, int64_t stats[ALEGO_STATIC_VERDICTS]) {
  if (!opts || !hits || !passes || n < 0 || (n > 0 && (!pts || !verdict)) || occ_opts_fault(opts)) return ALEGO_ERR_ARG;
  const alego_static_rule R = rule ? *rule : occ_static_rule_default();
  if (occ_static_rule_fault(&R) || (R.use_keep_below && !sensor_z)) return ALEGO_ERR_ARG;
  int64_t local[ALEGO_STATIC_VERDICTS] = {0, 0, 0, 0, 0, 0};
  occ_mark_host(occ_grid(opts), R, hits, passes, pts, sensor_z, n, verdict, local);
  if (stats) for (int k = 0; k < ALEGO_STATIC_VERDICTS; ++k) stats[k] = local[k];
  return 0;
}

int alego_loc_status(alego_handle* h, int slot, int32_t out[4]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!out) return ALEGO_ERR_ARG;
  return lm_host_loc_status(h->lm, slot, out, &h->err);
}

// ---- key-frame pass-through ---------------------------------------------------------------------------------------
int alego_lm_keyframe_count(alego_handle* h, int slot) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_keyframe_count(h->lm, slot);
}
int alego_lm_get_keyframe(alego_handle* h, int slot, int kf_id, alego_keyframe* out) {
  ALEGO_GATE_SLOT(h, slot);
  if (!out) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_lm_get_keyframe", MAPPING)) return r;
  return lm_host_get_keyframe(h->lm, slot, kf_id, out, &h->err);
}
int alego_lm_set_keypose(alego_handle* h, int slot, int kf_id, const float pose6[6]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!pose6) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_lm_set_keypose", MAPPING)) return r;
  return lm_host_set_keypose(h->lm, h->d, slot, kf_id, pose6, &h->err);
}
int alego_lm_reset_window(alego_handle* h, int slot) {
  ALEGO_GATE_SLOT(h, slot);
  if (int r = gate_need(h, "alego_lm_reset_window", MAPPING)) return r;
  return lm_host_reset_window(h->lm, slot, &h->err);
}
int alego_lm_apply_correction(alego_handle* h, int slot, const double rc[12]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!rc) return ALEGO_ERR_ARG;
  return lm_host_apply_correction(h->lm, h->d, slot, rc, &h->err);
}
int alego_lm_add_keyframe(alego_handle* h, int slot, const float pose6[6], const alego_point* corner, int32_t n_corner,
                          const alego_point* surf, int32_t n_surf, const alego_point* outlier, int32_t n_outlier) {
  ALEGO_GATE_SLOT(h, slot);
  if (!pose6) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_lm_add_keyframe", MAPPING)) return r;
  return lm_host_add_keyframe(h->lm, h->d, slot, pose6, corner, n_corner, surf, n_surf, outlier, n_outlier, &h->err);
}

// ---- the global map -------------------------------------------------------------------------------------------------
int alego_map_enable(alego_handle* h, int32_t max_keyframes, int32_t max_points) {
  ALEGO_GATE(h);
  if (max_keyframes <= 0 || max_points <= 0) return ALEGO_ERR_ARG;
  if (int r = gate_need(h, "alego_map_enable", NOT_STREAM_MODE | MAPPING)) return r;
  if (h->map_on) { h->err = "alego_map_enable: already enabled"; return ALEGO_ERR_ARG; }
  WAIT_ALL(h);
  if (int r = lm_host_map_enable(h->lm, max_keyframes, max_points, &h->err)) return r;
  h->map_on = true;
  return 0;
}
int alego_map_status(alego_handle* h, int slot, int32_t out[4]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!out) return ALEGO_ERR_ARG;
  return lm_host_map_status(h->lm, slot, out, &h->err);
}
int alego_map_set_keyposes(alego_handle* h, int slot, int32_t first, int32_t n, const float* poses6) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_map_set_keyposes(h->lm, slot, first, n, poses6, &h->err);
}
int alego_map_get_keyframe(alego_handle* h, int slot, int32_t id, alego_keyframe* out) {
  ALEGO_GATE_SLOT(h, slot);
  if (!out) return ALEGO_ERR_ARG;
  return lm_host_map_get_keyframe(h->lm, slot, id, out, &h->err);
}
int alego_map_assemble(alego_handle* h, int slot, int kinds, float leaf, alego_point* out, int32_t cap) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_map_assemble(h->lm, slot, kinds, leaf, out, cap, &h->err);
}
int alego_map_get_stamps(alego_handle* h, int slot, int32_t first, int32_t n, double* out) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_map_stamps(h->lm, slot, first, n, out, 0, &h->err);
}
int alego_map_set_stamps(alego_handle* h, int slot, int32_t first, int32_t n, const double* stamps) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_map_stamps(h->lm, slot, first, n, const_cast<double*>(stamps), 1, &h->err);
}
int alego_map_keyposes(alego_handle* h, int slot, alego_point* out, int32_t cap) {
  ALEGO_GATE_SLOT(h, slot);
  return lm_host_map_keyposes(h->lm, slot, out, cap, &h->err);
}
int alego_lm_get_local_map(alego_handle* h, int slot, alego_point* corner, int32_t corner_cap, alego_point* surf, int32_t surf_cap, int32_t n_out[2]) {
  ALEGO_GATE_SLOT(h, slot);
  if (!n_out || corner_cap < 0 || surf_cap < 0) return ALEGO_ERR_ARG;
  return lm_host_get_local_map(h->lm, slot, corner, corner_cap, surf, surf_cap, n_out, &h->err);
}
int alego_voxel_grid(alego_handle* h, const alego_point* pts, int32_t n, float leaf, alego_point* out, int32_t cap) {
  ALEGO_GATE(h);
  if (n < 0 || cap < 0 || (n > 0 && !pts) || !(leaf > 0.f)) return ALEGO_ERR_ARG;
  return lm_host_voxel_grid(h->lm, h->stream, pts, n, leaf, out, cap, &h->err);
}

int alego_debug_get(alego_handle* h, int slot, const char* name, void* out, int cap_bytes, int* count, int* dtype) {
  ALEGO_GATE_SLOT(h, slot);
  const DevCtx& d = h->d;
  int sc[SC_COUNT];
  DevTry c(__func__, &h->err);
  if (c.down(sc, scal_of(d, slot), stream_of(h, slot)).wait(stream_of(h, slot))) return c;
  const std::string s(name);
  if (s.rfind("la_", 0) == 0) {   // the appearance search: the descriptors / ring keys of the slot's archived frames described so far, as bytes
    const void* rsrc = nullptr;
    size_t bytes = 0;
    if (loop_app_debug_get(h->rl, slot, name, &rsrc, &bytes)) { h->err = std::string("debug_get: ") + name + " needs alego_loop_appearance_enable"; return ALEGO_ERR_ARG; }
    if ((size_t)cap_bytes < bytes) { h->err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
    if (c.took(dev_down_bytes(out, rsrc, bytes), "device read")) return c;
    *count = (int)bytes; *dtype = 3;
    return 0;
  }
  if (s.rfind("rl_", 0) == 0) {   // relocalisation: descriptors as bytes; "rl_stats": pairs evaluated by the second round / pairs in all of the last search
    if (s == "rl_stats") {
      if (cap_bytes < 8) { h->err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
      reloc_debug_stats(h->rl, (int*)out);
      *count = 2; *dtype = 2;
      return 0;
    }
    const void* rsrc = nullptr;
    size_t bytes = 0;
    if (reloc_debug_get(h->rl, slot, name, &rsrc, &bytes)) { h->err = std::string("debug_get: ") + name + " needs alego_reloc_enable"; return ALEGO_ERR_ARG; }
    if ((size_t)cap_bytes < bytes) { h->err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
    if (c.took(dev_down_bytes(out, rsrc, bytes), "device read")) return c;
    *count = (int)bytes; *dtype = 3;
    return 0;
  }
  if (s == "fe_cand_span") {   // sectors per fe_cand wavefront (0: the whole ring), the list entries of a sector
    if (cap_bytes < 8) { h->err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
    ((int*)out)[0] = fe_cand_span(d); ((int*)out)[1] = fe_sector_cap(d);
    *count = 2; *dtype = 2;
    return 0;
  }
  if (s == "fe_cand_counts" || s == "fe_cand_lists") {   // what fe_cand wrote for the slot's last scan, ring by ring: [ring][sector][2] i32 counts (sharp, flat) / [ring][sector][sector_cap][2] u32 (key, pay) as i32
    if (!fe_fused_eligible(d)) { h->err = "debug_get: " + s + " needs the fused feature extraction"; return ALEGO_ERR_ARG; }
    const bool lists = s == "fe_cand_lists";
    const size_t row = lists ? (size_t)d.P.n_sectors * fe_sector_cap(d) * sizeof(uint2) : (size_t)d.P.n_sectors * 2 * sizeof(int);
    const void* src = lists ? (const void*)st_cand_of(d, slot, 0) : (const void*)st_idx_of(d, slot, 0, F_LFLAT);
    const size_t pitch = lists ? (size_t)((const char*)st_cand_of(d, slot, 1) - (const char*)st_cand_of(d, slot, 0)) : (size_t)((const char*)st_idx_of(d, slot, 1, F_LFLAT) - (const char*)st_idx_of(d, slot, 0, F_LFLAT));
    if ((size_t)cap_bytes < row * d.NS) { h->err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
    HIP_TRY(h, hipMemcpy2D(out, row, src, pitch, row, d.NS, hipMemcpyDeviceToHost));
    *count = (int)(row * d.NS / 4); *dtype = 2;
    return 0;
  }
  const size_t base = (size_t)slot * d.N, M = sc[SC_M];
  const size_t fb = fbuf(slot, sc[SC_CUR]);  // buffer written by the last processed scan
  int fc[F_KINDS];
  if (c.down(fc, feat_cnt_of(d, fb))) return c;
  static const char* const cloud[F_KINDS] = {"sharp", "less_sharp", "flat", "less_flat"};
  struct Row { std::string name; const void* row; size_t n; int dtype; };   // dtype 0: f32, 1: f64, 2: i32, 3: u8
  std::vector<Row> tab = {
    {"range_img", d.range_img + base, (size_t)d.N, 0}, {"label_img", d.label_img + base, (size_t)d.N, 2}, {"flag_img", d.flag_img + base, (size_t)d.N, 3},
    {"owner", d.owner + base, (size_t)d.N, 2}, {"parent", d.parent + base, (size_t)d.N, 2},
    {"seg_cloud", d.seg_pts + base, M * 4, 0}, {"outlier", d.outlier + base, (size_t)sc[SC_NOUT] * 4, 0},
    {"imu_ptr", imu_ptr_of(d, slot), IMP_N, 2}, {"imu_ring", imu_ring_of(d, slot), imu_ring_n(), 1},
    {"seg_ground", d.seg_ground + base, M, 3}, {"seg_col", d.seg_col + base, M, 2}, {"seg_range", d.seg_range + base, M, 0},
    {"ring_start", ring_start_of(d, slot, 0), (size_t)d.NS, 2}, {"ring_end", ring_end_of(d, slot, 0), (size_t)d.NS, 2},
    {"orientation", ori_of(d, slot), ORI_N, 0}, {"scal", scal_of(d, slot), SC_COUNT, 2},
    {"curv_d", d.cd + base, M, 0}, {"picked_occl", d.picked0 + base, M, 3}, {"point_label", d.plabel + base, M, 2},
    {"lo_surf_corr", lo_corr_of(d, slot, 0), (size_t)fc[F_FLAT] * LC_W, 2}, {"lo_corner_corr", lo_corr_of(d, slot, 1), (size_t)fc[F_SHARP] * LC_W, 2},
    {"lo_state", lo_state_of(d, slot), LO_STATE_N, 1}, {"poses", poses_of(d, slot), PO_W, 1}};
  if (d.P.deskew_mode) tab.push_back({"undistorted", d.seg_dsk + base, (size_t)sc[SC_M_DSK] * 4, 0});
  for (int k = 0; k < F_KINDS; ++k) {
    tab.push_back({cloud[k], feat_of(d, k, fb), (size_t)fc[k] * 4, 0});
    if (k < F_LFLAT) tab.push_back({std::string(cloud[k]) + "_idx", feat_idx_of(d, k, fb), (size_t)fc[k], 2});
  }
  const Row* hit = nullptr;
  for (const Row& r : tab) if (r.name == s) hit = &r;
  if (!hit) return lm_host_debug_get(h->lm, slot, name, out, cap_bytes, count, dtype, &h->err);
  const void* src = hit->row;
  const size_t n = hit->n, esz = hit->dtype == 1 ? 8 : hit->dtype == 3 ? 1 : 4;
  const int dt = hit->dtype;
  if ((size_t)cap_bytes < n * esz) { h->err = "debug_get: buffer too small"; return ALEGO_ERR_CAPACITY; }
  if (c.took(dev_down_bytes(out, src, n * esz), "device read")) return c;
  *count = (int)n; *dtype = dt;
  return 0;
}

}  // extern "C"
