// examples/replay.cpp — the C ABI used from plain C++ (no Python, no ROS): what a host program that links libalego_mi355x.so looks like.
//
// Two sources of scans:
//   examples/replay [n_scans] [n_scan] [horizon_scan]
//       the synthetic S0/T0 stream (libalego_synth.so stands in for the sensor);
//   examples/replay --bag FILE.bag [--topic /lslidar_point_cloud] [--list] [--scans N] [--n-scan 16] [--horizon 4000] [--standalone]
//       a recorded rosbag (format 2.0; uncompressed, bz2 or lz4 chunks) read by the library's own reader: what
//       `rosbag play test_0515.bag` + `roslaunch alego test2.launch` do in the reference (README.md:33-37, launch/test2.launch:6-14).
//       --standalone selects the IP.cpp twin of ImageProjection: RFANS-16M ring table + removeClosedPointCloud(1.0 m)
//       (IP.cpp:77-104,117,142-172; utility.h:81); the default is the nodelet (imageProjection.cpp) on the reference geometry
//       16 x 4000 (utility.h:50-55).  --list prints the bag's topics and needs no GPU.
//   either source + --save-map DIR [--map-leaf L] [--map-frames N] [--map-points N]
//       keeps every key frame on the device (alego_map_enable, capacities per stream) and, at the end, writes saveMapCB's files
//       (laserMapping.cpp:826-874: keypose.pcd, corner.pcd, surf.pcd, outlier.pcd) and global.pcd, the cloud
//       visualizeGlobalMapThread publishes (:598-616), VoxelGrid(L)-filtered when --map-leaf is given.
//   either source + --loop-search EVERY
//       keeps the archive on too and calls alego_loop_search every EVERY scans (performLoopClosure, laserMapping.cpp:652-733, on the
//       device); every accepted constraint prints one line "loop: scan K slot S latest L closest C fitness F".  A host with a pose
//       graph would add the Between factor here and write the corrected poses back.
//   --loop-search EVERY + --gate CHI2 [--max-loops N]
//       the key-pose graph is on as well, and every found constraint is judged before it is added: alego_graph_check_loops gives the squared
//       Mahalanobis distance d2 of the edge against the covariance the graph predicts; one line "gate: scan K slot S
//       d2 D accepted A" follows the "loop:" line, and only an edge with d2 <= CHI2 goes to alego_graph_add_loops (ALEGO_GRAPH_CHI2_6_999 =
//       22.46 is the 0.999 quantile for 6 degrees of freedom).  Nothing is optimised or applied.
//   either source + --close-loops EVERY [--max-loops N]
//       the whole loop closure on the device: the key-pose graph next to the archive (alego_graph_enable), and every EVERY scans
//       alego_loop_search -> alego_graph_add_loops -> alego_graph_optimize with apply = 1 (correctPoses, :561-584).  Every applied
//       correction prints one line "closed: scan K slot S poses N loops L iterations I cost C0 -> C"; with --save-map the map comes
//       out at the corrected poses.
//   --loop-search / --close-loops + --appearance [--app-max-jump M] [--app-range R]
//       the radius search runs first; a slot for which it returns status 0 (no archived key pose within lc_search_radius: the drift may
//       exceed it) goes to alego_loop_search_appearance, which recognises the place from the clouds (alego_loop_appearance_enable with
//       max_range R, default the library's; M = its max_jump gate in metres, default off).  A closure accepted that way prints the same
//       line followed by " appearance D S": the descriptor distance and the yaw shift of the accepted candidate.
//   --loop-radius R
//       lc_search_radius of the radius search in metres (history_search_radius_, default 20): a small R leaves the revisits to --appearance.
//   either source + --align START2
//       a second slot of the same handle replays the source from scan START2 (a second session through the same site), both with the archive
//       and the appearance descriptors on.  At the end alego_map_align(src = slot 1, dst = slot 0) asks which rigid transform takes the second
//       archive into the frame of the first and prints one line "align: status S queries Q accepted A support K T t00 .. t23" (T row-major 3 x 4).
//   --align START2 + --merge
//       after an alignment with status 2 the second slot's archive is merged into the first's on the device: alego_map_merge(src = slot 1,
//       dst = slot 0) with the alignment's T, its hypotheses as cross edges and a loose seam (variances 0.01 rad^2 / 0.25 m^2), then
//       alego_graph_optimize with apply = 1 over the union (the key-pose graph is on for both slots).  One line "merge: status S frames F points P
//       loop_edges L cross_edges X optimise status O poses N loops M iterations I cost C0 -> C"; with --save-map the files hold the union.
//   either source + --thin DIST
//       after the run's end (or after --merge) alego_map_thin(slot 0, min_dist = DIST) removes the archived frames that lie closer than DIST
//       to a frame that stays.  One line "thin: status S frames N -> N' points P -> P'"; with --save-map the files hold the thinned map.
//       The newest recent_keyframe_num + 1 frames (50 + 1 by default; --recent-keyframes K sets the parameter) are resident and always stay.
//   either source + --localize [--loc-radius R]
//       map once, then localise in that map: the run above keeps the archive on; afterwards every archived key frame is pulled with
//       alego_map_get_keyframe, a SECOND handle is opened, alego_loc_enable hands it those frames, and the same scans are replayed through
//       it.  It never saves a key frame; every mapping frame registers against the map frames nearest to its pose.  The JSON line gains
//       "loc_map_t" (its final map pose) and "loc_max_dev" (the largest per-axis distance between the two runs' map poses).
//   --localize + --on-device
//       the mapping handle stays alive and alego_loc_enable_from_map hands its archive to the second handle on the device, no frame crossing to
//       the host; the printed poses equal those of --localize digit for digit, and the JSON line gains "loc_on_device": 1.
//   --localize + --relocalize [--reloc-start K] [--reloc-range R]
//       the localising handle's stream starts UNPLACED at scan K of the source (default: half way) — nothing tells the handle where it is.
//       alego_reloc_enable builds the map's descriptors (R = max_range, default the library's); after the stream's first mapping frame
//       alego_loc_relocalize with apply = 1 finds the place, verifies it by ICP and places the slot on the device.  The result is printed
//       as one line "reloc: {...}"; loc_max_dev then covers the scans after the placement, and the JSON line gains "reloc_status".
//   either source + --remap [EIG_MIN]
//       alego_remap_enable: LaserMapping's registration holds the directions its first evaluation does not observe (eigenvalue below EIG_MIN,
//       default 100) at the point the solve starts from.  Every key frame prints one line "remap: scan K status S n_held H
//       eig_min E" (the smallest eigenvalue of the information matrix at the point the solve started from).
//   either source + --regcov [--regcov-graph]
//       alego_regcov_enable: every mapping frame leaves the covariance of its scan-to-map registration on the device.
//       Every key frame prints one line "regcov: scan K status S rows R n_degenerate D eig_min E variance v0 .. v5" (the smallest eigenvalue of
//       the information matrix; rotation x y z in rad^2, then translation x y z in m^2).  --regcov-graph turns the archive and the key-pose
//       graph on as well and writes those variances into the odometry edges (opts.graph = 1): with --loop-search N --gate CHI2 the gate then
//       judges every found loop against noise the registrations measured instead of the constant default.
//   either source + --occupancy CELL DIR [--occ-range R]
//       keeps the archive on and, at the end (after --merge / --thin), casts every archived point as a ray from its key pose into an occupancy
//       grid on the device (alego_occ_enable / _integrate / _classify): square cells of CELL metres in x and y over the
//       key poses' bounding box plus R (max_range, default 30 m), ONE layer in z from 0.5 m below the lowest key pose to 1 m above the
//       highest, so that ground returns leave the layer from below and count as free space only.  Writes DIR/occupancy.pgm (P5; 254 free,
//       0 occupied, 205 unknown; the top row is the largest y, as map_server reads it) and DIR/occupancy.yaml, and prints one line
//       "occupancy: origin X Y Z cell CX CY CZ n NX NY NZ max_range R rays N short S truncated T culled C bad B updates U".
//   --occupancy CELL DIR + --inflate INSCRIBED RADIUS [SCALING]
//       the inflated cost map of that grid (alego_occ_costmap): costmap_2d's inflation layer with the robot's inscribed
//       radius, the inflation radius (metres) and the cost scaling factor (default 10) over the collapsed grid.  Writes DIR/costmap.pgm (P5,
//       maxval 255, the raw costs: 254 lethal, 253 inscribed, 255 unknown; rows as occupancy.pgm orders them) and prints one line
//       "costmap: r R sources A far B max_d2 C lethal D inscribed E unknown F" (R the radius in cells; sources, cells beyond it and the
//       largest squared distance within it, in cells).  Without --occupancy it is a usage error (exit status 2).
//   --save-map DIR + --static CELL [--occ-range R] [--static-keep-below Z] [--static-protect RADIUS]
//       the static map (alego_map_assemble_static): after --merge / --thin and the files above, a 3-D grid of cubes of CELL
//       metres over the key poses' bounding box plus R (default 30 m) in x and y and from 3 m below the lowest key pose to 3 m above the highest in
//       z takes every archived point as a ray (max_range = R); DIR/static.pcd is global.pcd (all kinds, --map-leaf applied) without the points
//       that lie in cells seen free: what moved while the map was made.  Z keeps every point whose sensor-frame z is below Z (ground returns),
//       RADIUS keeps points next to an occupied cell.  Prints one line
//       "static: kept_occupied A unknown B outside C below D neighbour E removed F of N".  Not together with --occupancy (one grid per handle).
// Every scan goes through ImageProjection -> LaserOdometry -> LaserMapping with one alego_scan_process call, as a single nodelet
// manager would run them (launch/test.launch:6-10); every new key frame is pulled across the boundary the way the reference's
// pose-graph thread reads cloud_keyposes_6d_ (laserMapping.cpp:586-596); one JSON line with the final poses is printed.
//
//   g++ -O2 -std=c++17 -Iinclude examples/replay.cpp -o examples/replay -La-lego-loam_amd -lalego_mi355x -lalego_synth
//       -Wl,-rpath,'$ORIGIN/../a-lego-loam_amd'                                  (__graft_entry__.build() does this)
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "alego_mi355x.h"

extern "C" int alego_synth_scan(const alego_params* P, int stream, long scan_index, int flags, alego_point* out, int cap);

int main(int argc, char** argv) {
  std::string bag_path, topic = "/lslidar_point_cloud", map_dir, occ_dir;
  double occ_cell = 0.0, occ_range = 30.0, static_cell = 0.0;
  bool inflate = false;
  alego_occ_inflation inflation = {0.0, 0.0, 10.0, 0, 0};
  alego_static_rule static_rule = {{1, 2, 1, 0}, 0, 0, 0.f, 0};
  float map_leaf = 0.f;
  int map_frames = 4096, map_points = 1 << 24, loop_every = 0, close_every = 0, max_loops = 16;
  bool list_only = false, standalone = false, localize = false, relocalize = false, appearance = false, merge = false, on_device = false, regcov = false, regcov_graph = false, remap = false;
  double remap_eig_min = 0.0;
  double gate_chi2 = -1.0, loc_radius = 0.0, reloc_range = 0.0, app_max_jump = 0.0, app_range = 0.0, loop_radius = 0.0, thin_dist = -1.0;
  long reloc_start = -1, align_start = -1;
  long max_scans = -1;
  int n_scan = 16, horizon = -1, recent_keyframes = 0;
  std::vector<const char*> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
    if (a == "--bag") bag_path = val();
    else if (a == "--topic") topic = val();
    else if (a == "--list") list_only = true;
    else if (a == "--standalone") standalone = true;
    else if (a == "--scans") max_scans = std::atol(val());
    else if (a == "--n-scan") n_scan = std::atoi(val());
    else if (a == "--horizon") horizon = std::atoi(val());
    else if (a == "--save-map") map_dir = val();
    else if (a == "--map-leaf") map_leaf = std::atof(val());
    else if (a == "--map-frames") map_frames = std::atoi(val());
    else if (a == "--map-points") map_points = std::atoi(val());
    else if (a == "--loop-search") loop_every = std::atoi(val());
    else if (a == "--gate") gate_chi2 = std::atof(val());
    else if (a == "--close-loops") close_every = std::atoi(val());
    else if (a == "--max-loops") max_loops = std::atoi(val());
    else if (a == "--appearance") appearance = true;
    else if (a == "--app-max-jump") app_max_jump = std::atof(val());
    else if (a == "--app-range") app_range = std::atof(val());
    else if (a == "--loop-radius") loop_radius = std::atof(val());
    else if (a == "--align") align_start = std::atol(val());
    else if (a == "--merge") merge = true;
    else if (a == "--thin") thin_dist = std::atof(val());
    else if (a == "--occupancy") { occ_cell = std::atof(val()); occ_dir = val(); }
    else if (a == "--occ-range") occ_range = std::atof(val());
    else if (a == "--inflate") {
      inflate = true; inflation.inscribed_radius = std::atof(val()); inflation.inflation_radius = std::atof(val());
      if (i + 1 < argc && (std::isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '.')) inflation.cost_scaling = std::atof(argv[++i]);
    }
    else if (a == "--static") static_cell = std::atof(val());
    else if (a == "--static-keep-below") { static_rule.use_keep_below = 1; static_rule.keep_below = (float)std::atof(val()); }
    else if (a == "--static-protect") static_rule.protect_radius = std::atoi(val());
    else if (a == "--recent-keyframes") recent_keyframes = std::atoi(val());
    else if (a == "--localize") localize = true;
    else if (a == "--on-device") on_device = true;
    else if (a == "--loc-radius") loc_radius = std::atof(val());
    else if (a == "--relocalize") relocalize = true;
    else if (a == "--reloc-start") reloc_start = std::atol(val());
    else if (a == "--reloc-range") reloc_range = std::atof(val());
    else if (a == "--regcov") regcov = true;
    else if (a == "--regcov-graph") regcov = regcov_graph = true;
    else if (a == "--remap") { remap = true; if (i + 1 < argc && (std::isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '.')) remap_eig_min = std::atof(argv[++i]); }
    else pos.push_back(argv[i]);
  }
  if (inflate && occ_dir.empty()) { std::fprintf(stderr, "--inflate needs --occupancy CELL DIR\n"); return 2; }
  alego_bag* bag = nullptr;
  long n_scans = pos.size() > 0 ? std::atol(pos[0]) : 40;
  if (!bag_path.empty()) {
    if (alego_bag_open(bag_path.c_str(), &bag) != ALEGO_OK) return 1;
    if (list_only) {
      for (int i = 0; i < alego_bag_topic_count(bag); ++i) {
        const char *t, *ty; int64_t n;
        alego_bag_topic_info(bag, i, &t, &ty, &n);
        std::printf("%-32s %-32s %lld\n", t, ty, (long long)n);
      }
      alego_bag_close(bag);
      return 0;
    }
    n_scans = (long)alego_bag_message_count(bag, topic.c_str());
    if (n_scans <= 0) { std::fprintf(stderr, "no messages on %s (try --list)\n", topic.c_str()); alego_bag_close(bag); return 1; }
    if (max_scans >= 0 && max_scans < n_scans) n_scans = max_scans;
    if (horizon < 0) horizon = 4000;           // the geometry compiled into the reference (utility.h:50-55)
  } else {
    if (pos.size() > 1) n_scan = std::atoi(pos[1]);
    horizon = pos.size() > 2 ? std::atoi(pos[2]) : (horizon < 0 ? 1800 : horizon);
  }
  alego_params P;
  alego_default_params(&P, n_scan, horizon);
  if (standalone) { P.laser_type = ALEGO_LASER_RFANS_16M; P.near_filter = 1; }
  if (loop_radius > 0.0) P.lc_search_radius = loop_radius;
  if (recent_keyframes > 0) P.recent_keyframe_num = recent_keyframes;
  if (alego_params_sizeof() != (int)sizeof(alego_params)) { std::fprintf(stderr, "header / library mismatch\n"); return 2; }
  const int N = P.n_scan * P.horizon_scan;
  const int cap_in = bag ? (1 << 20) : N;      // a driver may publish more returns than cells; the library takes at most N per scan
  std::vector<alego_point> pts(cap_in), kc(N), ks(N), ko(N);
  double stamp0 = 0.0;
  if (bag) {   // pcl::removeNaNFromPointCloud follows the message's is_dense (alego_params.input_is_dense): read it off the first message
    int32_t dense = 0;
    if (alego_bag_read_pc2(bag, topic.c_str(), 0, pts.data(), cap_in, &stamp0, &dense) < 0) { std::fprintf(stderr, "%s\n", alego_bag_last_error(bag)); alego_bag_close(bag); return 1; }
    P.input_is_dense = dense;
  }
  alego_handle* h = nullptr;
  if (int rc = alego_create(&P, /*device*/ 0, /*slots*/ align_start >= 0 ? 2 : 1, /*ring*/ 1, &h)) {
    std::fprintf(stderr, "alego_create failed (%d): there is no CPU fallback, an MI355X is required\n", rc);
    return 1;
  }
  if (!occ_dir.empty() && !(occ_cell > 0.0 && occ_range > 0.0)) { std::fprintf(stderr, "--occupancy needs a positive CELL (and --occ-range a positive R)\n"); alego_destroy(h); return 2; }
  if (static_cell != 0.0 && (map_dir.empty() || !occ_dir.empty() || !(static_cell > 0.0 && occ_range > 0.0))) {
    std::fprintf(stderr, "--static needs --save-map DIR and a positive CELL, and goes without --occupancy\n"); alego_destroy(h); return 2;
  }
  if ((!map_dir.empty() || !occ_dir.empty() || loop_every > 0 || close_every > 0 || localize || align_start >= 0 || thin_dist >= 0.0 || regcov_graph) && alego_map_enable(h, map_frames, map_points) != ALEGO_OK) {
    std::fprintf(stderr, "map_enable: %s\n", alego_last_error(h)); alego_destroy(h); return 1;
  }
  if (merge && align_start < 0) { std::fprintf(stderr, "--merge needs --align START2\n"); alego_destroy(h); return 2; }
  if (gate_chi2 >= 0.0 && loop_every <= 0) { std::fprintf(stderr, "--gate needs --loop-search EVERY\n"); alego_destroy(h); return 2; }
  if ((close_every > 0 || merge || gate_chi2 >= 0.0 || regcov_graph) && alego_graph_enable(h, merge ? std::max(max_loops, ALEGO_ALIGN_MAX_QUERIES) : max_loops, nullptr) != ALEGO_OK) {
    std::fprintf(stderr, "graph_enable: %s\n", alego_last_error(h)); alego_destroy(h); return 1;
  }
  if (remap) {
    alego_remap_opts mo{};
    mo.eig_min = remap_eig_min;
    if (alego_remap_enable(h, &mo) != ALEGO_OK) { std::fprintf(stderr, "remap_enable: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
  }
  if (regcov) {   // after the graph: graph = 1 needs it, and var_min defaults to its odometry variances
    alego_regcov_opts ro{};
    ro.graph = regcov_graph ? 1 : 0;
    if (alego_regcov_enable(h, &ro) != ALEGO_OK) { std::fprintf(stderr, "regcov_enable: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
  }
  if (((appearance && (loop_every > 0 || close_every > 0)) || align_start >= 0) && alego_loop_appearance_enable(h, app_range, 0.0 / 0.0) != ALEGO_OK) {
    std::fprintf(stderr, "loop_appearance_enable: %s\n", alego_last_error(h)); alego_destroy(h); return 1;
  }
  // the radius search first; with --appearance a slot it has no candidate for is searched by appearance.  app = " appearance D S" of a closure found that way
  auto find_loop = [&](int32_t slot, alego_loop_result* lr, std::string* app) -> int {
    app->clear();
    if (int rc = alego_loop_search(h, &slot, 1, lr)) return rc;
    if (!appearance || lr->status != 0) return ALEGO_OK;
    const alego_loop_app_opts ao{0, -1, 0, app_max_jump, 0.0};   // 0 / -1: the defaults (4 candidates, 1 verified)
    alego_loop_app_info ai{};
    if (int rc = alego_loop_search_appearance(h, &slot, 1, &ao, lr, &ai)) return rc;
    if (lr->status == 2) *app = " appearance " + std::to_string(ai.cand_dist[ai.verified]) + " " + std::to_string(ai.cand_shift[ai.verified]);
    return ALEGO_OK;
  };
  alego_pose odom{}, mapped{};
  int key_frames = 0, last_flags = 0, dropped = 0;
  float last_key_pose[6] = {0, 0, 0, 0, 0, 0};
  std::vector<alego_point> pts2(align_start >= 0 ? cap_in : 0);   // --align: the second slot's scan
  bool align_ended = false;
  std::vector<double> map_track;   // --localize: the mapping run's map pose of every scan (NaN for a dropped message)
  for (long k = 0; k < n_scans; ++k) {
    int n;
    double stamp = 0.1 * k;
    if (bag) {
      n = alego_bag_read_pc2(bag, topic.c_str(), k, pts.data(), cap_in, &stamp, nullptr);
      if (n < 0 || n > N) map_track.insert(map_track.end(), 3, 0.0 / 0.0);
      if (n < 0) { std::fprintf(stderr, "message %ld: %s\n", k, alego_bag_last_error(bag)); ++dropped; continue; }   // pcCB would warn and return
      if (n > N) { std::fprintf(stderr, "message %ld: %d points > n_scan * horizon_scan = %d (use --n-scan / --horizon)\n", k, n, N); ++dropped; continue; }
    } else {
      n = alego_synth_scan(&P, 0, k, 0, pts.data(), N);
    }
    alego_scan_in in{pts.data(), n, stamp};
    const int flags = alego_scan_process(h, 0, &in, /*IP | LO | LM*/ 7, nullptr, nullptr, &odom, &mapped);
    if (flags < 0) { std::fprintf(stderr, "scan %ld: %s\n", k, alego_last_error(h)); alego_destroy(h); return 1; }
    last_flags = flags;
    map_track.insert(map_track.end(), mapped.t, mapped.t + 3);
    if (align_start >= 0 && !align_ended) {   // the second session: slot 1, START2 scans further on, from buffers of its own
      const long k2 = align_start + k;
      double stamp2 = 0.1 * k;
      int n2;
      if (!bag) {
        n2 = alego_synth_scan(&P, 0, k2, 0, pts2.data(), N);
      } else if (k2 >= (long)alego_bag_message_count(bag, topic.c_str())) {
        std::fprintf(stderr, "align: the bag ends at message %ld: the second slot stops after %ld scans\n", k2, k);
        align_ended = true;
        n2 = -1;
      } else {
        n2 = alego_bag_read_pc2(bag, topic.c_str(), k2, pts2.data(), cap_in, &stamp2, nullptr);
        if (n2 < 0) std::fprintf(stderr, "message %ld (slot 1): %s\n", k2, alego_bag_last_error(bag));
        else if (n2 > N) std::fprintf(stderr, "message %ld (slot 1): %d points > n_scan * horizon_scan = %d\n", k2, n2, N);
      }
      if (n2 >= 0 && n2 <= N) {
        alego_scan_in in2{pts2.data(), n2, stamp2};
        alego_pose o2{}, m2{};
        if (alego_scan_process(h, 1, &in2, 7, nullptr, nullptr, &o2, &m2) < 0) { std::fprintf(stderr, "scan %ld (slot 1): %s\n", k2, alego_last_error(h)); alego_destroy(h); return 1; }
      }
    }
    if (flags & ALEGO_FLAG_LM_KEYFRAME) {   // saveKeyFramesAndFactor stored a frame: fetch it as the pose-graph thread would
      alego_keyframe kf{};
      kf.corner = kc.data(); kf.corner_cap = N; kf.surf = ks.data(); kf.surf_cap = N; kf.outlier = ko.data(); kf.outlier_cap = N;
      if (alego_lm_get_keyframe(h, 0, -1, &kf) < 0) { std::fprintf(stderr, "get_keyframe: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
      ++key_frames;
      for (int i = 0; i < 6; ++i) last_key_pose[i] = kf.pose[i];
      if (regcov) {   // the registration that produced this key frame: how well was it constrained?
        const int32_t slot = 0;
        alego_regcov rc{};
        if (alego_regcov_get(h, &slot, 1, &rc) != ALEGO_OK) { std::fprintf(stderr, "regcov_get: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
        std::printf("regcov: scan %ld status %d rows %d n_degenerate %d eig_min %.6g variance %.6g %.6g %.6g %.6g %.6g %.6g\n", k, rc.status, rc.n_edge + rc.n_plane,
                    rc.n_degenerate, rc.eigval[0], rc.variance[0], rc.variance[1], rc.variance[2], rc.variance[3], rc.variance[4], rc.variance[5]);
      }
      if (remap) {   // ... and which directions did it hold at its start?
        const int32_t slot = 0;
        alego_remap rm{};
        if (alego_remap_get(h, &slot, 1, &rm) != ALEGO_OK) { std::fprintf(stderr, "remap_get: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
        std::printf("remap: scan %ld status %d n_held %d eig_min %.6g\n", k, rm.status, rm.n_held, rm.eigval[0]);
      }
    }
    if (loop_every > 0 && (k + 1) % loop_every == 0) {
      const int32_t slot = 0;
      alego_loop_result lr{};
      std::string app;
      if (find_loop(slot, &lr, &app) != ALEGO_OK) { std::fprintf(stderr, "loop_search: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
      if (lr.status == 2) std::printf("loop: scan %ld slot %d latest %d closest %d fitness %.9g%s\n", k, slot, lr.latest_id, lr.closest_id, lr.fitness, app.c_str());
      if (lr.status == 2 && gate_chi2 >= 0.0) {   // judge the edge against the graph as it stands; add it only when it is believable
        alego_graph_check gc{};
        if (alego_graph_check_loops(h, &slot, 1, &lr, &gc) != ALEGO_OK) { std::fprintf(stderr, "graph_check_loops: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
        const bool accepted = gc.status == 1 && gc.d2 <= gate_chi2;
        std::printf("gate: scan %ld slot %d d2 %.9g accepted %d\n", k, slot, gc.d2, accepted ? 1 : 0);
        if (accepted && alego_graph_add_loops(h, &slot, 1, &lr) != ALEGO_OK) { std::fprintf(stderr, "graph_add_loops: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
      }
    }
    if (close_every > 0 && (k + 1) % close_every == 0) {   // search -> add the Between factor -> optimise and correct, all on the device
      const int32_t slot = 0;
      alego_loop_result lr{};
      alego_graph_result gr{};
      const alego_graph_opts go{0, 0.0, 1};
      std::string app;
      if (find_loop(slot, &lr, &app) != ALEGO_OK || alego_graph_add_loops(h, &slot, 1, &lr) != ALEGO_OK ||
          (lr.status == 2 && alego_graph_optimize(h, &slot, 1, &go, &gr) != ALEGO_OK)) {
        std::fprintf(stderr, "close loops: %s\n", alego_last_error(h)); alego_destroy(h); return 1;
      }
      if (gr.applied) std::printf("closed: scan %ld slot %d poses %d loops %d iterations %d cost %.9g -> %.9g%s\n", k, slot, gr.n_poses, gr.n_loops, gr.iterations, gr.cost0, gr.cost, app.c_str());
    }
  }
  if (align_start >= 0) {
    const int32_t src = 1, dst = 0;
    alego_map_align_result ar{};
    std::vector<alego_map_align_hyp> hyp(merge ? ALEGO_ALIGN_MAX_QUERIES : 0);
    if (alego_map_align(h, &src, &dst, 1, nullptr, &ar, merge ? hyp.data() : nullptr) != ALEGO_OK) { std::fprintf(stderr, "map_align: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
    std::printf("align: status %d queries %d accepted %d support %d T", ar.status, ar.n_queries, ar.n_accepted, ar.support);
    for (int i = 0; i < 12; ++i) std::printf(" %.9g", ar.T[i]);
    std::printf("\n");
    if (merge && ar.status == 2) {   // the two sessions become one map: append, tie by the hypotheses, optimise, correct
      const double seam[6] = {1e-2, 1e-2, 1e-2, 0.25, 0.25, 0.25};
      const alego_map_merge_opts mo{0.0, seam};
      alego_map_merge_result mr{};
      alego_graph_result gr{};
      const alego_graph_opts go{0, 0.0, 1};
      if (alego_map_merge(h, &src, &dst, 1, ar.T, &mo, hyp.data(), &mr) != ALEGO_OK || (mr.status == 2 && alego_graph_optimize(h, &dst, 1, &go, &gr) != ALEGO_OK)) {
        std::fprintf(stderr, "map_merge: %s\n", alego_last_error(h)); alego_destroy(h); return 1;
      }
      std::printf("merge: status %d frames %d points %d loop_edges %d cross_edges %d optimise status %d poses %d loops %d iterations %d cost %.9g -> %.9g\n",
                  mr.status, mr.frames, mr.points, mr.loop_edges, mr.cross_edges, gr.status, gr.n_poses, gr.n_loops, gr.iterations, gr.cost0, gr.cost);
    }
  }
  if (thin_dist >= 0.0) {   // after the run's end or the merge: frames closer than DIST to a frame that stays leave slot 0's archive (--save-map then writes the thinned map)
    const int32_t slot = 0;
    const alego_map_thin_opts to{thin_dist};
    alego_map_thin_result tr{};
    if (alego_map_thin(h, &slot, 1, &to, &tr) != ALEGO_OK) { std::fprintf(stderr, "map_thin: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
    std::printf("thin: status %d frames %d -> %d points %d -> %d\n", tr.status, tr.frames_before, tr.frames, tr.points_before, tr.points);
  }
  std::string loc_json;
  if (localize) {   // the second half: a fresh handle localises the same scans in the map the first one built
    int32_t st[4] = {0, 0, 0, 0};
    if (alego_map_status(h, 0, st) != ALEGO_OK) { std::fprintf(stderr, "map_status: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
    const int nf = st[0];
    std::vector<std::vector<alego_point>> clouds((size_t)nf * 3);
    std::vector<alego_kf_in> frames(nf);
    for (int i = 0; i < nf && !on_device; ++i) {
      alego_keyframe kf{};
      kf.corner = kc.data(); kf.corner_cap = N; kf.surf = ks.data(); kf.surf_cap = N; kf.outlier = ko.data(); kf.outlier_cap = N;
      if (alego_map_get_keyframe(h, 0, i, &kf) < 0) { std::fprintf(stderr, "map_get_keyframe: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
      clouds[i * 3 + 0].assign(kc.begin(), kc.begin() + kf.n_corner);
      clouds[i * 3 + 1].assign(ks.begin(), ks.begin() + kf.n_surf);
      clouds[i * 3 + 2].assign(ko.begin(), ko.begin() + kf.n_outlier);
      for (int a = 0; a < 6; ++a) frames[i].pose[a] = kf.pose[a];
      frames[i].corner = clouds[i * 3 + 0].data(); frames[i].n_corner = kf.n_corner;
      frames[i].surf = clouds[i * 3 + 1].data(); frames[i].n_surf = kf.n_surf;
      frames[i].outlier = clouds[i * 3 + 2].data(); frames[i].n_outlier = kf.n_outlier;
    }
    alego_handle* hl = nullptr;
    if (alego_create(&P, 0, 1, 1, &hl)) { std::fprintf(stderr, "alego_create (localising handle) failed\n"); alego_destroy(h); return 1; }
    // --on-device: the mapping handle stays alive and hands its archive over on the device; no frame comes to the host
    if ((on_device ? alego_loc_enable_from_map(hl, h, 0, loc_radius, 0) : alego_loc_enable(hl, frames.data(), nf, loc_radius)) != ALEGO_OK) {
      std::fprintf(stderr, "%s: %s\n", on_device ? "loc_enable_from_map" : "loc_enable", alego_last_error(hl)); alego_destroy(hl); alego_destroy(h); return 1;
    }
    if (relocalize && alego_reloc_enable(hl, reloc_range, 0.0 / 0.0) != ALEGO_OK) { std::fprintf(stderr, "reloc_enable: %s\n", alego_last_error(hl)); alego_destroy(hl); alego_destroy(h); return 1; }
    if (reloc_start < 0) reloc_start = n_scans / 2;
    int reloc_status = -1;   // -1: not asked for; 0: no verdict yet
    alego_pose lo{}, lm{};
    double max_dev = 0.0;
    for (long k = relocalize ? reloc_start : 0; k < n_scans; ++k) {
      int n;
      double stamp = 0.1 * k;
      if (bag) {
        n = alego_bag_read_pc2(bag, topic.c_str(), k, pts.data(), cap_in, &stamp, nullptr);
        if (n < 0 || n > N) continue;
      } else {
        n = alego_synth_scan(&P, 0, k, 0, pts.data(), N);
      }
      alego_scan_in in{pts.data(), n, stamp};
      const int flags = alego_scan_process(hl, 0, &in, 7, nullptr, nullptr, &lo, &lm);
      if (flags < 0) { std::fprintf(stderr, "localise scan %ld: %s\n", k, alego_last_error(hl)); alego_destroy(hl); alego_destroy(h); return 1; }
      if (relocalize && reloc_status <= 0) {   // unplaced: ask after every scan until the slot has had a mapping frame (status 0 before)
        const int32_t slot = 0;
        const alego_reloc_opts ro{0, -1, 1};   // the defaults (4 candidates, 1 verified) and apply
        alego_reloc_result rr{};
        if (alego_loc_relocalize(hl, &slot, 1, &ro, &rr) != ALEGO_OK) { std::fprintf(stderr, "relocalize: %s\n", alego_last_error(hl)); alego_destroy(hl); alego_destroy(h); return 1; }
        reloc_status = rr.status;
        if (rr.status > 0) {
          std::printf("reloc: {\"scan\": %ld, \"status\": %d, \"applied\": %d, \"verified\": %d, \"cand_id\": [", k, rr.status, rr.applied, rr.verified);
          for (int c = 0; c < rr.n_cand; ++c) std::printf("%s%d", c ? ", " : "", rr.cand_id[c]);
          std::printf("], \"cand_dist\": [");
          for (int c = 0; c < rr.n_cand; ++c) std::printf("%s%d", c ? ", " : "", rr.cand_dist[c]);
          std::printf("], \"cand_shift\": [");
          for (int c = 0; c < rr.n_cand; ++c) std::printf("%s%d", c ? ", " : "", rr.cand_shift[c]);
          std::printf("], \"converged\": %d, \"iterations\": %d, \"fitness\": %.17g, \"t_map\": [", rr.converged, rr.iterations, rr.fitness);
          for (int c = 0; c < 16; ++c) std::printf("%s%.9g", c ? ", " : "", rr.t_map[c]);
          std::printf("], \"params6\": [");
          for (int c = 0; c < 6; ++c) std::printf("%s%.17g", c ? ", " : "", rr.params6[c]);
          std::printf("]}\n");
        }
        continue;   // (the deviation is measured from the first scan after the placement)
      }
      for (int a = 0; a < 3; ++a) {
        const double dev = lm.t[a] - map_track[(size_t)k * 3 + a];
        if (!(std::fabs(dev) <= max_dev)) max_dev = std::fabs(dev);   // (a NaN sticks)
      }
    }
    char buf[320];
    int len = std::snprintf(buf, sizeof(buf), ", \"loc_frames\": %d, \"loc_map_t\": [%.17g, %.17g, %.17g], \"loc_max_dev\": %.9g", nf, lm.t[0], lm.t[1], lm.t[2], max_dev);
    if (relocalize) len += std::snprintf(buf + len, sizeof(buf) - len, ", \"reloc_status\": %d", reloc_status);
    if (on_device) std::snprintf(buf + len, sizeof(buf) - len, ", \"loc_on_device\": 1");
    loc_json = buf;
    alego_destroy(hl);
  }
  std::printf("{\"scans\": %ld, \"dropped\": %d, \"flags\": %d, \"key_frames\": %d, \"resident_key_frames\": %d, "
              "\"odom_t\": [%.17g, %.17g, %.17g], \"map_t\": [%.17g, %.17g, %.17g], \"map_params\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], "
              "\"last_key_pose\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g]%s}\n",
              n_scans, dropped, last_flags, key_frames, alego_lm_keyframe_count(h, 0), odom.t[0], odom.t[1], odom.t[2], mapped.t[0], mapped.t[1], mapped.t[2],
              mapped.params[0], mapped.params[1], mapped.params[2], mapped.params[3], mapped.params[4], mapped.params[5],
              last_key_pose[0], last_key_pose[1], last_key_pose[2], last_key_pose[3], last_key_pose[4], last_key_pose[5], loc_json.c_str());
  int rc = 0;
  if (!map_dir.empty()) {   // saveMapCB + the /laser_cloud_surround cloud, from the archive at the key poses that hold now
    struct { const char* name; int kinds; float leaf; } files[] = {
        {"corner.pcd", ALEGO_MAP_CORNER | ALEGO_MAP_FRAME_ID, 0.f}, {"surf.pcd", ALEGO_MAP_SURF | ALEGO_MAP_FRAME_ID, 0.f},
        {"outlier.pcd", ALEGO_MAP_OUTLIER | ALEGO_MAP_FRAME_ID, 0.f}, {"global.pcd", ALEGO_MAP_SURF | ALEGO_MAP_CORNER | ALEGO_MAP_OUTLIER, map_leaf}};
    std::vector<alego_point> cloud;
    int n = alego_map_keyposes(h, 0, nullptr, 0);
    if (n >= 0) { cloud.resize(n > 0 ? n : 1); n = alego_map_keyposes(h, 0, cloud.data(), n); }
    if (n < 0 || alego_write_pcd((map_dir + "/keypose.pcd").c_str(), cloud.data(), n) != ALEGO_OK) rc = 1;
    for (const auto& f : files) {
      if (rc) break;
      n = alego_map_assemble(h, 0, f.kinds, f.leaf, nullptr, 0);
      if (n >= 0) { cloud.resize(n > 0 ? n : 1); n = alego_map_assemble(h, 0, f.kinds, f.leaf, cloud.data(), n); }
      if (n < 0 || alego_write_pcd((map_dir + "/" + f.name).c_str(), cloud.data(), n) != ALEGO_OK) rc = 1;
    }
    int32_t st[4];
    if (!rc && alego_map_status(h, 0, st) == ALEGO_OK && st[1] > 0) std::fprintf(stderr, "map: %d key frames did not fit the archive (--map-frames / --map-points)\n", st[1]);
    if (rc) std::fprintf(stderr, "save map to %s: %s\n", map_dir.c_str(), alego_last_error(h));
  }
  if (static_cell > 0.0 && !rc) {   // the static map of slot 0's archive at the key poses that hold now
    std::vector<alego_point> kp;
    int n = alego_map_keyposes(h, 0, nullptr, 0);
    if (n > 0) { kp.resize(n); n = alego_map_keyposes(h, 0, kp.data(), n); }
    if (n <= 0) { std::fprintf(stderr, "static: no key frame archived\n"); alego_destroy(h); return 1; }
    double lo[3] = {kp[0].x, kp[0].y, kp[0].z}, hi[3] = {kp[0].x, kp[0].y, kp[0].z};
    for (int i = 1; i < n; ++i) {
      const double v[3] = {kp[i].x, kp[i].y, kp[i].z};
      for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    }
    alego_occ_opts oo{};
    for (int a = 0; a < 3; ++a) {
      const double margin = a < 2 ? occ_range : 3.0;
      oo.cell[a] = static_cell;
      oo.origin[a] = std::floor((lo[a] - margin) / static_cell) * static_cell;
      oo.n[a] = (int32_t)std::ceil((hi[a] + margin - oo.origin[a]) / static_cell);
    }
    oo.min_range = 0.0; oo.max_range = occ_range;
    const int all = ALEGO_MAP_SURF | ALEGO_MAP_CORNER | ALEGO_MAP_OUTLIER;
    int64_t st[ALEGO_STATIC_VERDICTS];
    std::vector<alego_point> cloud(1);
    int m = -1;
    if (alego_occ_enable(h, &oo) == ALEGO_OK && alego_occ_integrate(h, 0, 0, -1, all, nullptr) == ALEGO_OK) {
      m = alego_map_assemble_static(h, 0, all, map_leaf, &static_rule, nullptr, 0, nullptr);
      if (m >= 0) { cloud.resize(m > 0 ? m : 1); m = alego_map_assemble_static(h, 0, all, map_leaf, &static_rule, cloud.data(), m, st); }
    }
    if (m < 0) { std::fprintf(stderr, "static: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
    if (alego_write_pcd((map_dir + "/static.pcd").c_str(), cloud.data(), m) != ALEGO_OK) { std::fprintf(stderr, "static: cannot write to %s\n", map_dir.c_str()); rc = 1; }
    long long total = 0;
    for (int k = 0; k < ALEGO_STATIC_VERDICTS; ++k) total += st[k];
    std::printf("static: kept_occupied %lld unknown %lld outside %lld below %lld neighbour %lld removed %lld of %lld\n", (long long)st[ALEGO_STATIC_OCCUPIED],
                (long long)st[ALEGO_STATIC_UNKNOWN], (long long)st[ALEGO_STATIC_OUTSIDE], (long long)st[ALEGO_STATIC_BELOW], (long long)st[ALEGO_STATIC_NEIGHBOUR],
                (long long)st[ALEGO_STATIC_REMOVED], total);
  }
  if (!occ_dir.empty() && !rc) {   // the occupancy grid of slot 0's archive at the key poses that hold now
    std::vector<alego_point> kp;
    int n = alego_map_keyposes(h, 0, nullptr, 0);
    if (n > 0) { kp.resize(n); n = alego_map_keyposes(h, 0, kp.data(), n); }
    if (n <= 0) { std::fprintf(stderr, "occupancy: no key frame archived\n"); alego_destroy(h); return 1; }
    double lo[3] = {kp[0].x, kp[0].y, kp[0].z}, hi[3] = {kp[0].x, kp[0].y, kp[0].z};
    for (int i = 1; i < n; ++i) {
      const double v[3] = {kp[i].x, kp[i].y, kp[i].z};
      for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    }
    alego_occ_opts oo{};
    for (int a = 0; a < 2; ++a) {
      oo.cell[a] = occ_cell;
      oo.origin[a] = std::floor((lo[a] - occ_range) / occ_cell) * occ_cell;
      oo.n[a] = (int32_t)std::ceil((hi[a] + occ_range - oo.origin[a]) / occ_cell);
    }
    oo.origin[2] = lo[2] - 0.5; oo.cell[2] = hi[2] + 1.0 - oo.origin[2]; oo.n[2] = 1;
    oo.min_range = 0.0; oo.max_range = occ_range;
    int64_t st[ALEGO_OCC_STATS];
    std::vector<int8_t> cls((size_t)oo.n[0] * oo.n[1]);
    if (alego_occ_enable(h, &oo) != ALEGO_OK || alego_occ_integrate(h, 0, 0, -1, ALEGO_MAP_SURF | ALEGO_MAP_CORNER | ALEGO_MAP_OUTLIER, st) != ALEGO_OK ||
        alego_occ_classify(h, nullptr, 1, cls.data()) != ALEGO_OK) { std::fprintf(stderr, "occupancy: %s\n", alego_last_error(h)); alego_destroy(h); return 1; }
    std::printf("occupancy: origin %.17g %.17g %.17g cell %.17g %.17g %.17g n %d %d %d max_range %.17g rays %lld short %lld truncated %lld culled %lld bad %lld updates %lld\n",
                oo.origin[0], oo.origin[1], oo.origin[2], oo.cell[0], oo.cell[1], oo.cell[2], oo.n[0], oo.n[1], oo.n[2], oo.max_range, (long long)st[ALEGO_OCC_RAYS],
                (long long)st[ALEGO_OCC_SHORT], (long long)st[ALEGO_OCC_TRUNCATED], (long long)st[ALEGO_OCC_CULLED], (long long)st[ALEGO_OCC_BAD], (long long)st[ALEGO_OCC_UPDATES]);
    std::vector<unsigned char> img(cls.size());
    for (int y = 0; y < oo.n[1]; ++y)   // the image's top row is the grid's last
      for (int x = 0; x < oo.n[0]; ++x) {
        const int8_t c = cls[(size_t)(oo.n[1] - 1 - y) * oo.n[0] + x];
        img[(size_t)y * oo.n[0] + x] = c == 100 ? 0 : (c == 0 ? 254 : 205);
      }
    FILE* f = std::fopen((occ_dir + "/occupancy.pgm").c_str(), "wb");
    bool ok = f != nullptr;
    if (ok) { ok = std::fprintf(f, "P5\n%d %d\n255\n", oo.n[0], oo.n[1]) > 0 && std::fwrite(img.data(), 1, img.size(), f) == img.size(); ok = std::fclose(f) == 0 && ok; }
    f = ok ? std::fopen((occ_dir + "/occupancy.yaml").c_str(), "w") : nullptr;
    if (f) {
      ok = std::fprintf(f, "image: occupancy.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0.0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n", occ_cell, oo.origin[0], oo.origin[1]) > 0;
      ok = std::fclose(f) == 0 && ok;
    } else {
      ok = false;
    }
    if (!ok) { std::fprintf(stderr, "occupancy: cannot write to %s\n", occ_dir.c_str()); rc = 1; }
    if (inflate && ok) {   // the inflated cost map of the collapsed grid
      std::vector<uint8_t> cost(cls.size());
      std::vector<uint8_t> table((size_t)4095 * 4095 + 1);   // the largest table there is: the library says how much of it the parameters use
      const int n_table = alego_occ_cost_table_host(occ_cell, &inflation, table.data(), (int32_t)table.size());
      if (n_table < 1) { std::fprintf(stderr, "--inflate: INSCRIBED <= RADIUS, both and SCALING not negative, RADIUS at most 4095 cells\n"); alego_destroy(h); return 2; }
      const int r = (int)std::lround(std::sqrt((double)(n_table - 1)));   // n_table = r r + 1
      const alego_occ_dist_opts dopt = {1, 0, r, 0};
      int64_t ds[ALEGO_EDT_STATS];
      if (alego_occ_costmap(h, nullptr, 1, 0, &inflation, cost.data()) != ALEGO_OK || alego_occ_distance(h, nullptr, &dopt, nullptr, ds) != ALEGO_OK) {
        std::fprintf(stderr, "costmap: %s\n", alego_last_error(h)); alego_destroy(h); return 1;
      }
      long long lethal = 0, inscribed = 0, unknown = 0;
      for (uint8_t c : cost) { lethal += c == 254; inscribed += c == 253; unknown += c == 255; }
      std::printf("costmap: r %d sources %lld far %lld max_d2 %lld lethal %lld inscribed %lld unknown %lld\n", r, (long long)ds[ALEGO_EDT_SOURCES],
                  (long long)ds[ALEGO_EDT_FAR_CELLS], (long long)ds[ALEGO_EDT_MAX_D2], lethal, inscribed, unknown);
      for (int y = 0; y < oo.n[1]; ++y)
        for (int x = 0; x < oo.n[0]; ++x) img[(size_t)y * oo.n[0] + x] = cost[(size_t)(oo.n[1] - 1 - y) * oo.n[0] + x];
      f = std::fopen((occ_dir + "/costmap.pgm").c_str(), "wb");
      ok = f != nullptr;
      if (ok) { ok = std::fprintf(f, "P5\n%d %d\n255\n", oo.n[0], oo.n[1]) > 0 && std::fwrite(img.data(), 1, img.size(), f) == img.size(); ok = std::fclose(f) == 0 && ok; }
      if (!ok) { std::fprintf(stderr, "costmap: cannot write to %s\n", occ_dir.c_str()); rc = 1; }
    }
  }
  alego_destroy(h);
  if (bag) alego_bag_close(bag);
  return rc;
}
