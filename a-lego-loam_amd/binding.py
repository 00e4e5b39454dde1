"""ctypes binding of the C ABI in include/alego_mi355x.h (libalego_mi355x.so).

Host-side mirror of the reference's node interface: `Handle.ip_process` ~ ImageProjection::pcCB,
`Handle.lo_process` ~ LaserOdometry::mainLoop body, `Handle.lm_process` ~ LaserMapping::mainLoop
body, `Handle.scan_process` = the three chained on the device.  There is no CPU fallback: loading
fails loudly if the HIP library is missing and `Handle()` raises if no gfx950 device is visible.
"""
import ctypes as C
import os

import numpy as np

from .params import AlegoParams, AlegoPoint

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_DT = {0: np.float32, 1: np.float64, 2: np.int32, 3: np.uint8}

# every symbol include/alego_mi355x.h declares
EXPORTS = [
    "alego_create", "alego_destroy", "alego_last_error", "alego_device_count", "alego_params_sizeof",
    "alego_ip_process", "alego_lo_process", "alego_lm_process", "alego_scan_process",
    "alego_batch_load", "alego_batch_run", "alego_synchronize", "alego_batch_get_pose", "alego_batch_get_counts",
    "alego_stream", "alego_stream_groups", "alego_stream_plan", "alego_profile_enable", "alego_profile_report", "alego_set_lo_params", "alego_set_lm_params", "alego_debug_get", "alego_debug_voxel", "alego_debug_atan2f",
    "alego_lo_push_imu", "alego_lo_get_undistorted", "alego_pose_o2b", "alego_trajectory_enable", "alego_trajectory_get", "alego_debug_check_guards", "alego_debug_math", "alego_debug_std_sort", "alego_debug_eval_blocks", "alego_debug_transform_to_start", "alego_debug_set_option",
    "alego_lm_keyframe_count", "alego_lm_get_keyframe", "alego_lm_set_keypose", "alego_lm_reset_window", "alego_lm_apply_correction",
    "alego_lm_add_keyframe", "alego_pc2_to_points", "alego_replay_create", "alego_replay_load", "alego_replay_assign",
    "alego_dist_unique_id", "alego_dist_init", "alego_dist_shutdown", "alego_dist_allreduce_probe", "alego_stream_setup", "alego_stream_run",
    "alego_loop_detect", "alego_loop_closure_icp",
    "alego_bag_open", "alego_bag_close", "alego_bag_last_error", "alego_bag_topic_count", "alego_bag_topic_info", "alego_bag_message_count",
    "alego_bag_read_raw", "alego_bag_read_pc2", "alego_handle_lock", "alego_handle_unlock",
    "alego_map_enable", "alego_map_status", "alego_map_set_keyposes", "alego_map_get_keyframe", "alego_map_assemble", "alego_map_keyposes",
    "alego_lm_get_local_map", "alego_voxel_grid", "alego_write_pcd",
    "alego_map_get_stamps", "alego_map_set_stamps", "alego_loop_search", "alego_loop_constraint", "alego_debug_nn1",
    "alego_graph_enable", "alego_graph_status", "alego_graph_get_edges", "alego_graph_set_edges", "alego_graph_add_loops", "alego_graph_add_edge",
    "alego_graph_optimize", "alego_graph_get_estimate", "alego_graph_residuals",
    "alego_graph_marginals", "alego_graph_check_edges", "alego_graph_check_loops", "alego_graph_covariance_host", "alego_graph_check_host",
    "alego_loc_select", "alego_loc_enable", "alego_loc_status", "alego_loc_enable_from_map", "alego_loc_update_from_map",
    "alego_reloc_enable", "alego_loc_relocalize", "alego_reloc_descriptor", "alego_reloc_match", "alego_debug_reloc_search",
    "alego_loop_appearance_enable", "alego_loop_search_appearance", "alego_loop_appearance_candidates",
    "alego_map_align", "alego_map_align_queries", "alego_map_align_consensus", "alego_map_align_poses",
    "alego_map_move", "alego_map_merge", "alego_map_align_edge", "alego_map_merge_edges",
    "alego_map_thin", "alego_map_thin_select", "alego_map_thin_edges", "alego_debug_thin_select",
    "alego_regcov_enable", "alego_regcov_get", "alego_regcov_host", "alego_regcov_normal_host", "alego_debug_regcov",
    "alego_remap_enable", "alego_remap_get", "alego_remap_host", "alego_remap_step_host", "alego_debug_remap_solve",
    "alego_occ_enable", "alego_occ_clear", "alego_occ_integrate", "alego_occ_get", "alego_occ_classify", "alego_occ_ray_host", "alego_occ_integrate_host",
    "alego_occ_classify_host", "alego_debug_occ_piece", "alego_occ_mark", "alego_map_assemble_static", "alego_occ_mark_host",
    "alego_occ_set", "alego_occ_distance", "alego_occ_costmap", "alego_occ_distance_host", "alego_occ_cost_table_host", "alego_occ_costmap_host",
]

REPLAY_PINGPONG = 0x100
REPLAY_BAG = 0x200
MAP_SURF, MAP_CORNER, MAP_OUTLIER, MAP_FRAME_ID = 1, 2, 4, 8
ERR_CAPACITY, ERR_ARG = -3, -4
OCC_RAYS, OCC_SHORT, OCC_TRUNCATED, OCC_CULLED, OCC_BAD, OCC_UPDATES, OCC_STATS = 0, 1, 2, 3, 4, 5, 6   # ALEGO_OCC_*
OCC_SKIP_SHORT, OCC_SKIP_CULLED, OCC_SKIP_BAD = -10, -11, -12
STATIC_OCCUPIED, STATIC_UNKNOWN, STATIC_OUTSIDE, STATIC_BELOW, STATIC_NEIGHBOUR, STATIC_REMOVED, STATIC_VERDICTS = 0, 1, 2, 3, 4, 5, 6   # ALEGO_STATIC_*
OCC_FAR = 0xFFFFFFFF                                                    # ALEGO_OCC_FAR
EDT_SOURCES, EDT_FAR_CELLS, EDT_MAX_D2, EDT_STATS = 0, 1, 2, 3          # ALEGO_EDT_*
RELOC_MAX_CAND = 8
RELOC_SECTORS, RELOC_RINGS = 60, 20
ALIGN_MAX_QUERIES = 32
ALIGN_TOL_TRANS, ALIGN_TOL_ROT = 0.24, 0.0165   # ALEGO_ALIGN_TOL_TRANS, ALEGO_ALIGN_TOL_ROT
MERGE_COPY_ITEM = 1024                          # ALEGO_MERGE_COPY_ITEM
FLAG_LO_INIT, FLAG_FEW_SURF, FLAG_FEW_CORNER, FLAG_LM_SKIPPED, FLAG_LM_FEW_FEATURES, FLAG_LM_KEYFRAME = 1, 2, 4, 8, 16, 32


class ScanIn(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("n", C.c_int32), ("stamp", C.c_double)]


class SegOut(C.Structure):
    _fields_ = [("seg", C.c_void_p), ("seg_cap", C.c_int32), ("m", C.c_int32),
                ("ground", C.c_void_p), ("col", C.c_void_p), ("range", C.c_void_p),
                ("ring_start", C.c_void_p), ("ring_end", C.c_void_p), ("orientation", C.c_float * 3),
                ("outlier", C.c_void_p), ("outlier_cap", C.c_int32), ("n_outlier", C.c_int32),
                ("label_image", C.c_void_p), ("stamp", C.c_double)]


class FeatOut(C.Structure):
    _fields_ = [("sharp", C.c_void_p), ("sharp_cap", C.c_int32), ("n_sharp", C.c_int32),
                ("less_sharp", C.c_void_p), ("less_sharp_cap", C.c_int32), ("n_less_sharp", C.c_int32),
                ("flat", C.c_void_p), ("flat_cap", C.c_int32), ("n_flat", C.c_int32),
                ("less_flat", C.c_void_p), ("less_flat_cap", C.c_int32), ("n_less_flat", C.c_int32),
                ("point_label", C.c_void_p)]


class Pose(C.Structure):
    _fields_ = [("t", C.c_double * 3), ("q", C.c_double * 4), ("params", C.c_double * 6), ("valid", C.c_int32)]

    def as_dict(self):
        return dict(t=np.array(self.t[:]), q=np.array(self.q[:]), params=np.array(self.params[:]), valid=int(self.valid))


def pose_o2b(t, q, tf_b2l):
    """alego_pose_o2b: (t, q = w x y z) of /odom -> /laser and the 4 x 4 base_link -> laser mount -> (t, q) of /odom -> /base_link (LO.cpp:588-608)"""
    a, b = Pose(), Pose()
    a.t[:] = list(t); a.q[:] = list(q)
    m = np.ascontiguousarray(tf_b2l, np.float64).reshape(16)
    rc = lib().alego_pose_o2b(C.byref(a), m.ctypes.data, C.byref(b))
    if rc != 0:
        raise AlegoError(f"alego_pose_o2b failed ({rc})")
    return np.array(b.t[:]), np.array(b.q[:])


class KeyFrame(C.Structure):
    _fields_ = [("id", C.c_int32), ("pose", C.c_float * 6),
                ("corner", C.c_void_p), ("corner_cap", C.c_int32), ("n_corner", C.c_int32),
                ("surf", C.c_void_p), ("surf_cap", C.c_int32), ("n_surf", C.c_int32),
                ("outlier", C.c_void_p), ("outlier_cap", C.c_int32), ("n_outlier", C.c_int32)]


class KfIn(C.Structure):
    _fields_ = [("pose", C.c_float * 6), ("corner", C.c_void_p), ("n_corner", C.c_int32), ("surf", C.c_void_p), ("n_surf", C.c_int32),
                ("outlier", C.c_void_p), ("n_outlier", C.c_int32)]


class IcpResult(C.Structure):
    _fields_ = [("converged", C.c_int32), ("iterations", C.c_int32), ("n_source", C.c_int32), ("n_target", C.c_int32),
                ("fitness", C.c_double), ("correction", C.c_float * 16)]


class LoopResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("latest_id", C.c_int32), ("closest_id", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("n_source", C.c_int32), ("n_target", C.c_int32), ("fitness", C.c_double), ("correction", C.c_float * 16),
                ("t_correct", C.c_float * 16), ("between", C.c_double * 12), ("noise_variance", C.c_double)]


def _slot_list(slots, pairs=False):
    """a list of slots as (int32 array, count); with pairs, a list of (src, dst) pairs as (src array, dst array, count)"""
    a = np.ascontiguousarray(slots, np.int32).reshape((-1, 2) if pairs else -1)
    return (np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), a.shape[0]) if pairs else (a, a.shape[0])


def _loop_result(r):
    return dict(status=int(r.status), latest_id=int(r.latest_id), closest_id=int(r.closest_id), converged=int(r.converged),
                iterations=int(r.iterations), n_source=int(r.n_source), n_target=int(r.n_target), fitness=float(r.fitness),
                T=np.array(r.correction[:], np.float32).reshape(4, 4), t_correct=np.array(r.t_correct[:], np.float32).reshape(4, 4),
                between=np.array(r.between[:], np.float64).reshape(3, 4), noise_variance=float(r.noise_variance))


class RelocOpts(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("verify", C.c_int32), ("apply", C.c_int32)]


class RelocResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_cand", C.c_int32), ("cand_id", C.c_int32 * 8), ("cand_dist", C.c_int32 * 8), ("cand_shift", C.c_int32 * 8),
                ("verified", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32), ("n_source", C.c_int32), ("n_target", C.c_int32),
                ("applied", C.c_int32), ("fitness", C.c_double), ("correction", C.c_float * 16), ("guess6", C.c_float * 6), ("t_map", C.c_float * 16),
                ("rc", C.c_double * 12), ("params6", C.c_double * 6)]


class LoopAppOpts(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("verify", C.c_int32), ("max_dist", C.c_int32), ("max_jump", C.c_double), ("fitness_max", C.c_double)]


class LoopAppInfo(C.Structure):
    _fields_ = [("n_eligible", C.c_int32), ("n_cand", C.c_int32), ("cand_id", C.c_int32 * 8), ("cand_dist", C.c_int32 * 8), ("cand_shift", C.c_int32 * 8),
                ("verified", C.c_int32), ("guess6", C.c_float * 6), ("icp_final", C.c_float * 16)]


class MapAlignOpts(C.Structure):
    _fields_ = [("n_queries", C.c_int32), ("n_cand", C.c_int32), ("max_dist", C.c_int32), ("min_support", C.c_int32), ("fitness_max", C.c_double),
                ("tol_trans", C.c_double), ("tol_rot", C.c_double)]


class MapAlignHyp(C.Structure):
    _fields_ = [("src_frame", C.c_int32), ("dst_frame", C.c_int32), ("dist", C.c_int32), ("shift", C.c_int32), ("tried", C.c_int32), ("accepted", C.c_int32),
                ("converged", C.c_int32), ("iterations", C.c_int32), ("n_source", C.c_int32), ("n_target", C.c_int32), ("support", C.c_int32), ("inlier", C.c_int32),
                ("fitness", C.c_double), ("guess6", C.c_float * 6), ("icp_final", C.c_float * 16), ("T", C.c_float * 16)]


class MapAlignResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_queries", C.c_int32), ("n_accepted", C.c_int32), ("best", C.c_int32), ("support", C.c_int32), ("T", C.c_double * 12)]


class MapMergeOpts(C.Structure):
    _fields_ = [("stamp_offset", C.c_double), ("seam_variance", C.c_void_p)]


class MapMergeResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("frames", C.c_int32), ("points", C.c_int32), ("loop_edges", C.c_int32), ("cross_edges", C.c_int32)]


class MapThinOpts(C.Structure):
    _fields_ = [("min_dist", C.c_double)]


class MapThinResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("frames_before", C.c_int32), ("frames", C.c_int32), ("points_before", C.c_int32), ("points", C.c_int32)]


class OccOpts(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("cell", C.c_double * 3), ("n", C.c_int32 * 3), ("pad", C.c_int32), ("min_range", C.c_double), ("max_range", C.c_double)]


class OccRule(C.Structure):
    _fields_ = [("min_hits", C.c_int32), ("hit_weight", C.c_int32), ("pass_weight", C.c_int32), ("pad", C.c_int32)]


class StaticRule(C.Structure):
    _fields_ = [("occ", OccRule), ("protect_radius", C.c_int32), ("use_keep_below", C.c_int32), ("keep_below", C.c_float), ("pad", C.c_int32)]


class OccDistOpts(C.Structure):
    _fields_ = [("collapse_z", C.c_int32), ("unknown_is_obstacle", C.c_int32), ("max_cells", C.c_int32), ("pad", C.c_int32)]


class OccInflation(C.Structure):
    _fields_ = [("inscribed_radius", C.c_double), ("inflation_radius", C.c_double), ("cost_scaling", C.c_double), ("inflate_unknown", C.c_int32), ("pad", C.c_int32)]


class GraphEdge(C.Structure):
    _fields_ = [("frm", C.c_int32), ("to", C.c_int32), ("between", C.c_double * 12), ("variance", C.c_double * 6)]


class GraphOpts(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("step_tol", C.c_double), ("apply", C.c_int32)]


class GraphResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("n_poses", C.c_int32), ("n_loops", C.c_int32), ("applied", C.c_int32),
                ("cost0", C.c_double), ("cost", C.c_double), ("last_step", C.c_double)]


class GraphCovResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_poses", C.c_int32), ("n_loops", C.c_int32), ("pad", C.c_int32)]


class GraphCheck(C.Structure):
    _fields_ = [("status", C.c_int32), ("pad", C.c_int32), ("d2", C.c_double), ("error", C.c_double * 6), ("cov", C.c_double * 36)]


class RegCovOpts(C.Structure):
    _fields_ = [("sigma0", C.c_double), ("scale", C.c_double), ("eig_min", C.c_double), ("lambda_rel_floor", C.c_double),
                ("var_min", C.c_double * 6), ("var_max", C.c_double * 6), ("graph", C.c_int32), ("pad", C.c_int32)]


class RegCov(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_edge", C.c_int32), ("n_plane", C.c_int32), ("n_degenerate", C.c_int32), ("frame", C.c_int32), ("pad", C.c_int32),
                ("cost", C.c_double), ("sigma2", C.c_double), ("info", C.c_double * 36), ("eigval", C.c_double * 6), ("eigvec", C.c_double * 36),
                ("cov", C.c_double * 36), ("variance", C.c_double * 6)]


def regcov_opts(sigma0=0.0, scale=0.0, eig_min=0.0, lambda_rel_floor=0.0, var_min=None, var_max=None, graph=0):
    """alego_regcov_opts; a field left at 0 takes the library's default"""
    o = RegCovOpts()
    o.sigma0, o.scale, o.eig_min, o.lambda_rel_floor, o.graph = float(sigma0), float(scale), float(eig_min), float(lambda_rel_floor), int(graph)
    if var_min is not None:
        o.var_min[:] = [float(v) for v in var_min]
    if var_max is not None:
        o.var_max[:] = [float(v) for v in var_max]
    return o


def _record_out(r, shapes):
    """a record structure as a dict; shapes: field -> None (an int), () (a double) or the shape of an array of doubles"""
    get = lambda v, sh: int(v) if sh is None else float(v) if sh == () else np.array(v[:], np.float64).reshape(sh)  # noqa: E731
    return {f: get(getattr(r, f), sh) for f, sh in shapes.items()}


def _record_host(name, Rec, shapes, acc28, params6, n_edge, n_plane, opts):
    """a host twin's (acc28, params6, counts, opts) -> record call, the record as a dict"""
    a, p = np.ascontiguousarray(acc28, np.float64).reshape(28), np.ascontiguousarray(params6, np.float64).reshape(6)
    out = Rec()
    rc = getattr(lib(), name)(a.ctypes.data, p.ctypes.data, int(n_edge), int(n_plane), None if opts is None else C.byref(opts), C.byref(out))
    if rc != 0:
        raise AlegoError(f"{name} failed ({rc})")
    return _record_out(out, shapes)


_REGCOV_SHAPES = dict(status=None, n_edge=None, n_plane=None, n_degenerate=None, frame=None, cost=(), sigma2=(), info=(6, 6), eigval=(6,), eigvec=(6, 6), cov=(6, 6), variance=(6,))


def regcov_host(acc28, params6, n_edge, n_plane, opts=None):
    """alego_regcov_host (host only): the record of 28 normal-equation scalars at params6 as a dict"""
    return _record_host("alego_regcov_host", RegCov, _REGCOV_SHAPES, acc28, params6, n_edge, n_plane, opts)


def regcov_normal_host(params6, edge_rows9, plane_rows7, huber):
    """alego_regcov_normal_host (host only): the 28 scalars of rows (a, b, p) (n, 9) and (n, d, p) (m, 7) at params6"""
    p = np.ascontiguousarray(params6, np.float64).reshape(6)
    e, s = np.ascontiguousarray(edge_rows9, np.float64).reshape(-1, 9), np.ascontiguousarray(plane_rows7, np.float64).reshape(-1, 7)
    acc = np.zeros(28)
    rc = lib().alego_regcov_normal_host(p.ctypes.data, e.ctypes.data if len(e) else None, len(e), s.ctypes.data if len(s) else None, len(s), float(huber), acc.ctypes.data)
    if rc != 0:
        raise AlegoError(f"alego_regcov_normal_host failed ({rc})")
    return acc


class RemapOpts(C.Structure):
    _fields_ = [("eig_min", C.c_double)]


class Remap(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_held", C.c_int32), ("frame", C.c_int32), ("pad", C.c_int32),
                ("start", C.c_double * 6), ("eigval", C.c_double * 6), ("eigvec", C.c_double * 36), ("proj", C.c_double * 36)]


def remap_opts(eig_min=0.0):
    """alego_remap_opts; 0 takes the library's default (100)"""
    o = RemapOpts()
    o.eig_min = float(eig_min)
    return o


_REMAP_SHAPES = dict(status=None, n_held=None, frame=None, start=(6,), eigval=(6,), eigvec=(6, 6), proj=(6, 6))


def remap_host(acc28, params6, n_edge, n_plane, opts=None):
    """alego_remap_host (host only): the projector of 28 normal-equation scalars at params6 as a dict"""
    return _record_host("alego_remap_host", Remap, _REMAP_SHAPES, acc28, params6, n_edge, n_plane, opts)


def remap_step_host(H21, g6, scale6, radius, proj36=None):
    """alego_remap_step_host (host only): one lm_step at x = 0 -> (valid, step in parameter space (6,), model cost change)"""
    H, g, sc = (np.ascontiguousarray(v, np.float64).reshape(n) for v, n in ((H21, 21), (g6, 6), (scale6, 6)))
    P = None if proj36 is None else np.ascontiguousarray(proj36, np.float64).reshape(36)
    step, mcc = np.zeros(6), C.c_double(0.0)
    rc = lib().alego_remap_step_host(H.ctypes.data, g.ctypes.data, sc.ctypes.data, float(radius), None if P is None else P.ctypes.data, step.ctypes.data, C.byref(mcc))
    if rc < 0:
        raise AlegoError(f"alego_remap_step_host failed ({rc})")
    return bool(rc), step, mcc.value


def _graph_checks_out(out, n):
    return [dict(status=int(r.status), d2=float(r.d2), error=np.array(r.error[:], np.float64), cov=np.array(r.cov[:], np.float64).reshape(6, 6)) for r in out[:n]]


GRAPH_CHI2_6_999 = 22.457744484825323   # ALEGO_GRAPH_CHI2_6_999
GRAPH_MAX_LOOPS = 64
GRAPH_MAX_ITERS, GRAPH_STEP_TOL = 20, 1e-9   # ALEGO_GRAPH_MAX_ITERS, ALEGO_GRAPH_STEP_TOL


def graph_edges(frm, to, between, variance):
    """a ctypes array of alego_graph_edge from arrays: from (n,) (-1 = prior), to (n,), between (n, 3, 4), variance (n, 6)"""
    frm = np.asarray(frm, np.int64).reshape(-1)
    to = np.asarray(to, np.int64).reshape(-1)
    b = np.ascontiguousarray(between, np.float64).reshape(-1, 12)
    v = np.ascontiguousarray(variance, np.float64).reshape(-1, 6)
    out = (GraphEdge * max(len(frm), 1))()
    for i in range(len(frm)):
        out[i].frm, out[i].to = int(frm[i]), int(to[i])
        out[i].between[:] = b[i].tolist()
        out[i].variance[:] = v[i].tolist()
    return out


def graph_covariance_host(poses12, frm, to, between, variance, pairs=()):
    """alego_graph_covariance_host (host only): marginals (n_poses, 6, 6) and Sigma_ij (n_pairs, 6, 6) of a graph whose chain edges come first"""
    X = np.ascontiguousarray(poses12, np.float64).reshape(-1, 12)
    n = len(np.asarray(frm).reshape(-1))
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    marg, pair = np.zeros((X.shape[0], 36)), np.zeros((max(len(pr), 1), 36))
    rc = lib().alego_graph_covariance_host(X.ctypes.data, X.shape[0], graph_edges(frm, to, between, variance), n, pr.ctypes.data, len(pr), marg.ctypes.data, pair.ctypes.data)
    if rc != 0:
        raise AlegoError(f"alego_graph_covariance_host failed ({rc})")
    return marg.reshape(-1, 6, 6), pair[:len(pr)].reshape(-1, 6, 6)


def graph_check_host(poses12, frm, to, between, variance, cand_frm, cand_to, cand_between, cand_variance):
    """alego_graph_check_host (host only): one dict (status, d2, error (6,), cov (6, 6)) per candidate edge"""
    X = np.ascontiguousarray(poses12, np.float64).reshape(-1, 12)
    n, nc = len(np.asarray(frm).reshape(-1)), len(np.asarray(cand_frm).reshape(-1))
    out = (GraphCheck * max(nc, 1))()
    rc = lib().alego_graph_check_host(X.ctypes.data, X.shape[0], graph_edges(frm, to, between, variance), n,
                                      graph_edges(cand_frm, cand_to, cand_between, cand_variance), nc, out)
    if rc != 0:
        raise AlegoError(f"alego_graph_check_host failed ({rc})")
    return _graph_checks_out(out, nc)


def _graph_edges_out(e, n):
    return dict(frm=np.array([e[i].frm for i in range(n)], np.int64), to=np.array([e[i].to for i in range(n)], np.int64),
                between=np.array([e[i].between[:] for i in range(n)], np.float64).reshape(n, 3, 4),
                variance=np.array([e[i].variance[:] for i in range(n)], np.float64).reshape(n, 6))


def graph_residuals(poses12, frm, to, between, variance):
    """alego_graph_residuals (host only): whitened errors (n, 6), d / d delta_from (n, 6, 6), d / d delta_to (n, 6, 6)"""
    X = np.ascontiguousarray(poses12, np.float64).reshape(-1, 12)
    n = len(np.asarray(frm).reshape(-1))
    e = graph_edges(frm, to, between, variance)
    r, jf, jt = np.zeros((max(n, 1), 6)), np.zeros((max(n, 1), 36)), np.zeros((max(n, 1), 36))
    rc = lib().alego_graph_residuals(X.ctypes.data, X.shape[0], e, n, r.ctypes.data, jf.ctypes.data, jt.ctypes.data)
    if rc != 0:
        raise AlegoError(f"alego_graph_residuals failed ({rc})")
    return r[:n], jf[:n].reshape(n, 6, 6), jt[:n].reshape(n, 6, 6)


class Pc2Field(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint32), ("datatype", C.c_uint8), ("count", C.c_uint32)]


def lib_path():
    # ALEGO_LIB: a development build of the same library (e.g. with -DALEGO_TIMING for tools/*_timing.py)
    return os.environ.get("ALEGO_LIB") or os.path.join(_HERE, "libalego_mi355x.so")


def lib():
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: the HIP extension is not built (run __graft_entry__.build()); "
                               "there is no CPU fallback")
        L = C.CDLL(path)
        L.alego_create.restype = C.c_int
        L.alego_create.argtypes = [C.POINTER(AlegoParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.alego_destroy.argtypes = [C.c_void_p]
        L.alego_last_error.restype = C.c_char_p
        L.alego_last_error.argtypes = [C.c_void_p]
        L.alego_device_count.restype = C.c_int
        L.alego_params_sizeof.restype = C.c_int
        L.alego_ip_process.restype = C.c_int
        L.alego_ip_process.argtypes = [C.c_void_p, C.POINTER(ScanIn), C.POINTER(SegOut)]
        L.alego_lo_process.restype = C.c_int
        L.alego_lo_process.argtypes = [C.c_void_p, C.POINTER(SegOut), C.POINTER(FeatOut), C.POINTER(Pose)]
        L.alego_lm_process.restype = C.c_int
        L.alego_lm_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                       C.POINTER(Pose), C.POINTER(Pose)]
        L.alego_scan_process.restype = C.c_int
        L.alego_scan_process.argtypes = [C.c_void_p, C.c_int, C.POINTER(ScanIn), C.c_int, C.POINTER(SegOut),
                                         C.POINTER(FeatOut), C.POINTER(Pose), C.POINTER(Pose)]
        L.alego_batch_load.restype = C.c_int
        L.alego_batch_load.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int32]
        L.alego_batch_run.restype = C.c_int
        L.alego_batch_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.alego_synchronize.restype = C.c_int
        L.alego_synchronize.argtypes = [C.c_void_p]
        L.alego_batch_get_pose.restype = C.c_int
        L.alego_batch_get_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(Pose), C.POINTER(Pose)]
        L.alego_batch_get_counts.restype = C.c_int
        L.alego_batch_get_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.alego_profile_enable.restype = C.c_int
        L.alego_profile_enable.argtypes = [C.c_void_p, C.c_int]
        L.alego_profile_report.restype = C.c_int
        L.alego_profile_report.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.alego_stream.restype = C.c_void_p
        L.alego_stream.argtypes = [C.c_void_p]
        L.alego_stream_groups.restype = C.c_int
        L.alego_stream_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.alego_stream_plan.restype = C.c_int
        L.alego_stream_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.alego_set_lo_params.restype = C.c_int
        L.alego_set_lo_params.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.alego_set_lm_params.restype = C.c_int
        L.alego_set_lm_params.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.alego_debug_get.restype = C.c_int
        L.alego_debug_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.alego_debug_voxel.restype = C.c_int
        L.alego_debug_voxel.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
        L.alego_debug_atan2f.restype = C.c_int
        L.alego_debug_atan2f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.alego_trajectory_enable.restype = C.c_int
        L.alego_trajectory_enable.argtypes = [C.c_void_p, C.c_int32]
        L.alego_trajectory_get.restype = C.c_int
        L.alego_trajectory_get.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p]
        L.alego_lo_push_imu.restype = C.c_int
        L.alego_lo_push_imu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32]
        L.alego_lo_get_undistorted.restype = C.c_int
        L.alego_lo_get_undistorted.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32]
        L.alego_pose_o2b.restype = C.c_int
        L.alego_pose_o2b.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_debug_check_guards.restype = C.c_int
        L.alego_debug_check_guards.argtypes = [C.c_char_p, C.c_int]
        L.alego_debug_std_sort.restype = C.c_int
        L.alego_debug_std_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.alego_debug_math.restype = C.c_int
        L.alego_debug_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.alego_debug_eval_blocks.restype = C.c_int
        L.alego_debug_eval_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_debug_transform_to_start.restype = C.c_int
        L.alego_debug_transform_to_start.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.alego_debug_set_option.restype = C.c_int
        L.alego_debug_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.alego_lm_keyframe_count.restype = C.c_int
        L.alego_lm_keyframe_count.argtypes = [C.c_void_p, C.c_int]
        L.alego_lm_get_keyframe.restype = C.c_int
        L.alego_lm_get_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(KeyFrame)]
        L.alego_lm_set_keypose.restype = C.c_int
        L.alego_lm_set_keypose.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.alego_lm_reset_window.restype = C.c_int
        L.alego_lm_reset_window.argtypes = [C.c_void_p, C.c_int]
        L.alego_lm_apply_correction.restype = C.c_int
        L.alego_lm_apply_correction.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.alego_lm_add_keyframe.restype = C.c_int
        L.alego_lm_add_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.alego_pc2_to_points.restype = C.c_int
        L.alego_pc2_to_points.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                          C.POINTER(Pc2Field), C.c_int, C.c_void_p, C.c_int32]
        L.alego_replay_create.restype = C.c_int
        L.alego_replay_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.alego_replay_load.restype = C.c_int
        L.alego_replay_load.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int32]
        L.alego_replay_assign.restype = C.c_int
        L.alego_replay_assign.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.alego_dist_unique_id.restype = C.c_int
        L.alego_dist_unique_id.argtypes = [C.c_char_p]
        L.alego_dist_init.restype = C.c_int
        L.alego_dist_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
        L.alego_dist_shutdown.restype = C.c_int
        L.alego_dist_shutdown.argtypes = [C.c_void_p]
        L.alego_dist_allreduce_probe.restype = C.c_int
        L.alego_dist_allreduce_probe.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.alego_stream_setup.restype = C.c_int
        L.alego_stream_setup.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.alego_stream_run.restype = C.c_int
        L.alego_stream_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.alego_loop_detect.restype = C.c_int
        L.alego_loop_detect.argtypes = [C.POINTER(AlegoParams), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.alego_loop_closure_icp.restype = C.c_int
        L.alego_loop_closure_icp.argtypes = [C.c_void_p, C.POINTER(KfIn), C.POINTER(KfIn), C.c_int32, C.POINTER(IcpResult), C.c_void_p, C.c_int32]
        L.alego_handle_lock.restype = C.c_int
        L.alego_handle_lock.argtypes = [C.c_void_p]
        L.alego_handle_unlock.restype = C.c_int
        L.alego_handle_unlock.argtypes = [C.c_void_p]
        L.alego_bag_open.restype = C.c_int
        L.alego_bag_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.alego_bag_close.restype = None
        L.alego_bag_close.argtypes = [C.c_void_p]
        L.alego_bag_last_error.restype = C.c_char_p
        L.alego_bag_last_error.argtypes = [C.c_void_p]
        L.alego_bag_topic_count.restype = C.c_int
        L.alego_bag_topic_count.argtypes = [C.c_void_p]
        L.alego_bag_topic_info.restype = C.c_int
        L.alego_bag_topic_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
        L.alego_bag_message_count.restype = C.c_int64
        L.alego_bag_message_count.argtypes = [C.c_void_p, C.c_char_p]
        L.alego_bag_read_raw.restype = C.c_int
        L.alego_bag_read_raw.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.alego_bag_read_pc2.restype = C.c_int
        L.alego_map_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.alego_map_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.alego_map_set_keyposes.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p]
        L.alego_map_get_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.POINTER(KeyFrame)]
        L.alego_map_assemble.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int32]
        L.alego_map_keyposes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32]
        L.alego_lm_get_local_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.alego_voxel_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int32]
        L.alego_map_get_stamps.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p]
        L.alego_map_set_stamps.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p]
        L.alego_loop_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(LoopResult)]
        L.alego_loop_constraint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_debug_nn1.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.alego_graph_enable.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.alego_graph_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.alego_graph_get_edges.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int32, C.POINTER(GraphEdge)]
        L.alego_graph_set_edges.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.POINTER(GraphEdge)]
        L.alego_graph_add_loops.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(LoopResult)]
        L.alego_graph_add_edge.argtypes = [C.c_void_p, C.c_int, C.POINTER(GraphEdge), C.c_void_p]
        L.alego_graph_optimize.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(GraphOpts), C.POINTER(GraphResult)]
        L.alego_graph_get_estimate.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p]
        L.alego_graph_residuals.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GraphEdge), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_graph_marginals.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(GraphCovResult)]
        L.alego_graph_check_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(GraphEdge), C.POINTER(GraphCheck)]
        L.alego_graph_check_loops.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(LoopResult), C.POINTER(GraphCheck)]
        L.alego_graph_covariance_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GraphEdge), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.alego_graph_check_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GraphEdge), C.c_int32, C.POINTER(GraphEdge), C.c_int32, C.POINTER(GraphCheck)]
        L.alego_regcov_enable.argtypes = [C.c_void_p, C.POINTER(RegCovOpts)]
        L.alego_regcov_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RegCov)]
        L.alego_regcov_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RegCovOpts), C.POINTER(RegCov)]
        L.alego_regcov_normal_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
        L.alego_debug_regcov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(RegCov)]
        L.alego_remap_enable.argtypes = [C.c_void_p, C.POINTER(RemapOpts)]
        L.alego_remap_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Remap)]
        L.alego_remap_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RemapOpts), C.POINTER(Remap)]
        L.alego_remap_step_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.alego_debug_remap_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Remap)]
        L.alego_loc_select.restype = C.c_int
        L.alego_loc_select.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]
        L.alego_loc_enable.argtypes = [C.c_void_p, C.POINTER(KfIn), C.c_int32, C.c_double]
        L.alego_loc_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.alego_loc_enable_from_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int32]
        L.alego_loc_update_from_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.alego_reloc_enable.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.alego_loc_relocalize.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RelocOpts), C.POINTER(RelocResult)]
        L.alego_reloc_descriptor.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.alego_reloc_match.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.alego_debug_reloc_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_loop_appearance_enable.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.alego_loop_search_appearance.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(LoopAppOpts), C.POINTER(LoopResult), C.POINTER(LoopAppInfo)]
        L.alego_loop_appearance_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_map_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MapAlignOpts), C.POINTER(MapAlignResult), C.POINTER(MapAlignHyp)]
        L.alego_map_align_queries.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        L.alego_map_align_consensus.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.POINTER(C.c_int32)]
        L.alego_map_align_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.alego_map_move.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.alego_map_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(MapMergeOpts), C.POINTER(MapAlignHyp), C.POINTER(MapMergeResult)]
        L.alego_map_align_edge.argtypes = [C.POINTER(MapAlignHyp), C.c_void_p, C.c_int32, C.POINTER(GraphEdge)]
        L.alego_map_merge_edges.argtypes = [C.POINTER(GraphEdge), C.c_int32, C.POINTER(GraphEdge), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(GraphEdge), C.POINTER(GraphEdge)]
        L.alego_map_thin.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MapThinOpts), C.POINTER(MapThinResult)]
        L.alego_map_thin_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
        L.alego_map_thin_edges.argtypes = [C.POINTER(GraphEdge), C.c_int32, C.POINTER(GraphEdge), C.c_int32, C.c_void_p, C.POINTER(GraphEdge), C.POINTER(GraphEdge)]
        L.alego_debug_thin_select.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
        L.alego_occ_enable.argtypes = [C.c_void_p, C.POINTER(OccOpts)]
        L.alego_occ_clear.argtypes = [C.c_void_p]
        L.alego_occ_integrate.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_void_p]
        L.alego_occ_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_occ_classify.argtypes = [C.c_void_p, C.POINTER(OccRule), C.c_int, C.c_void_p]
        L.alego_debug_occ_piece.argtypes = [C.c_void_p, C.c_int32]
        L.alego_occ_ray_host.argtypes = [C.POINTER(OccOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.alego_occ_integrate_host.argtypes = [C.POINTER(OccOpts), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_occ_classify_host.argtypes = [C.POINTER(OccOpts), C.POINTER(OccRule), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.alego_occ_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.alego_occ_distance.argtypes = [C.c_void_p, C.POINTER(OccRule), C.POINTER(OccDistOpts), C.c_void_p, C.c_void_p]
        L.alego_occ_costmap.argtypes = [C.c_void_p, C.POINTER(OccRule), C.c_int, C.c_int, C.POINTER(OccInflation), C.c_void_p]
        L.alego_occ_distance_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p]
        L.alego_occ_cost_table_host.argtypes = [C.c_double, C.POINTER(OccInflation), C.c_void_p, C.c_int32]
        L.alego_occ_costmap_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
        L.alego_occ_mark.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(StaticRule), C.c_void_p, C.c_int32, C.c_void_p]
        L.alego_map_assemble_static.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(StaticRule), C.c_void_p, C.c_int32, C.c_void_p]
        L.alego_occ_mark_host.argtypes = [C.POINTER(OccOpts), C.POINTER(StaticRule), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.alego_write_pcd.argtypes = [C.c_char_p, C.c_void_p, C.c_int32]
        L.alego_bag_read_pc2.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        if L.alego_params_sizeof() != C.sizeof(AlegoParams):
            raise RuntimeError("alego_params layout mismatch between params.py and include/alego_params.h")
        _lib = L
    return _lib


class AlegoError(RuntimeError):
    pass


DIST_ID_BYTES = 128


def dist_unique_id() -> bytes:
    """rank 0: the RCCL unique id every rank passes to Handle.dist_init (ncclGetUniqueId)"""
    buf = C.create_string_buffer(DIST_ID_BYTES)
    rc = lib().alego_dist_unique_id(buf)
    if rc != 0:
        raise AlegoError(f"alego_dist_unique_id failed ({rc})")
    return buf.raw


def check_guards():
    """(count, report) of damaged allocation guards; count = -1 unless ALEGO_DEBUG_CANARY is set"""
    buf = C.create_string_buffer(4096)
    return lib().alego_debug_check_guards(buf, 4096), buf.value.decode(errors="replace")


def write_pcd(path, pts):
    """alego_write_pcd: PCD v0.7, DATA binary, FIELDS x y z intensity"""
    a = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    rc = lib().alego_write_pcd(os.fsencode(path), a.ctypes.data, a.shape[0])
    if rc != 0:
        raise AlegoError(f"alego_write_pcd({path}) failed ({rc})")


def loop_detect(params, keyposes6, stamps, cur_xyz):
    """detectLoopClosure's closest_history_frame_id_ (host code of the library; -1 = no candidate)"""
    kp = np.ascontiguousarray(keyposes6, np.float32).reshape(-1, 6)
    t = np.ascontiguousarray(stamps, np.float64)
    c = np.ascontiguousarray(cur_xyz, np.float64)
    return int(lib().alego_loop_detect(C.byref(params), kp.ctypes.data, t.ctypes.data, kp.shape[0], c.ctypes.data))


def loc_select(keyposes6, xyz, radius, k):
    """alego_loc_select: the window a localising slot at f32 position xyz selects from the map's key poses (ids ascending; host code of the library)"""
    kp = np.ascontiguousarray(keyposes6, np.float32).reshape(-1, 6)
    p = np.ascontiguousarray(xyz, np.float32).reshape(3)
    ids = np.empty(max(int(k), 1), np.int32)
    n = int(lib().alego_loc_select(kp.ctypes.data, kp.shape[0], p.ctypes.data, float(radius), int(k), ids.ctypes.data))
    if n < 0:
        raise AlegoError(f"alego_loc_select failed ({n})")
    return ids[:n].copy()


def reloc_descriptor(pts, max_range=0.0, z_offset=float("nan")):
    """alego_reloc_descriptor: (descriptor (60, 20) u8 [sector][ring], ring key (20,) u16) of a sensor-frame cloud (host code of the library)"""
    a = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    d = np.zeros((RELOC_SECTORS, RELOC_RINGS), np.uint8)
    k = np.zeros(RELOC_RINGS, np.uint16)
    rc = lib().alego_reloc_descriptor(a.ctypes.data, a.shape[0], float(max_range), float(z_offset), d.ctypes.data, k.ctypes.data)
    if rc != 0:
        raise AlegoError(f"alego_reloc_descriptor failed ({rc})")
    return d, k


def reloc_match(q, m):
    """alego_reloc_match: (D, shift) of two descriptors — the brute force over all 60 shifts (host code of the library)"""
    a = np.ascontiguousarray(q, np.uint8).reshape(RELOC_SECTORS * RELOC_RINGS)
    b = np.ascontiguousarray(m, np.uint8).reshape(RELOC_SECTORS * RELOC_RINGS)
    d, sh = C.c_int32(), C.c_int32()
    rc = lib().alego_reloc_match(a.ctypes.data, b.ctypes.data, C.byref(d), C.byref(sh))
    if rc != 0:
        raise AlegoError(f"alego_reloc_match failed ({rc})")
    return int(d.value), int(sh.value)


def loop_appearance_candidates(desc, keyposes6, stamps, min_time_gap, max_jump=0.0, max_dist=0, n_cand=4):
    """alego_loop_appearance_candidates: (ids, dists, shifts) of the candidates of the newest frame among the older ones (host code of the library)"""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, RELOC_SECTORS * RELOC_RINGS)
    kp = np.ascontiguousarray(keyposes6, np.float32).reshape(-1, 6)
    st = np.ascontiguousarray(stamps, np.float64).reshape(-1)
    assert kp.shape[0] == d.shape[0] == st.shape[0]
    ids, dists, shifts = (np.zeros(RELOC_MAX_CAND, np.int32) for _ in range(3))
    k = lib().alego_loop_appearance_candidates(d.ctypes.data, kp.ctypes.data, st.ctypes.data, d.shape[0], float(min_time_gap), float(max_jump), int(max_dist),
                                               int(n_cand), ids.ctypes.data, dists.ctypes.data, shifts.ctypes.data)
    if k < 0:
        raise AlegoError(f"alego_loop_appearance_candidates failed ({k})")
    return ids[:k].copy(), dists[:k].copy(), shifts[:k].copy()


def map_align_queries(n_frames, n_queries=0):
    """alego_map_align_queries: the source frames alego_map_align queries in an archive of n_frames (host code of the library)"""
    fr = np.zeros(ALIGN_MAX_QUERIES, np.int32)
    q = lib().alego_map_align_queries(int(n_frames), int(n_queries), fr.ctypes.data)
    if q < 0:
        raise AlegoError(f"alego_map_align_queries failed ({q})")
    return fr[:q].copy()


def map_align_consensus(T, src_pos, fitness, accepted, tol_trans=0.0, tol_rot=0.0):
    """alego_map_align_consensus: (support (n,), best) of n hypotheses T (n, 4, 4) with query positions src_pos (n, 3) (host code of the library)"""
    T = np.ascontiguousarray(T, np.float32).reshape(-1, 16)
    p = np.ascontiguousarray(src_pos, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(fitness, np.float64).reshape(-1)
    a = np.ascontiguousarray(accepted, np.int32).reshape(-1)
    n = T.shape[0]
    assert p.shape[0] == f.shape[0] == a.shape[0] == n
    sup, best = np.zeros(max(n, 1), np.int32), C.c_int32(-2)
    rc = lib().alego_map_align_consensus(T.ctypes.data, p.ctypes.data, f.ctypes.data, a.ctypes.data, n, float(tol_trans), float(tol_rot), sup.ctypes.data, C.byref(best))
    if rc != 0:
        raise AlegoError(f"alego_map_align_consensus failed ({rc})")
    return sup[:n].copy(), int(best.value)


def map_align_poses(T, poses6):
    """alego_map_align_poses: the key poses (n, 6) moved by T (3 x 4 or 4 x 4, f64) (host code of the library)"""
    T12 = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1)[:12])
    kp = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
    out = np.zeros_like(kp)
    rc = lib().alego_map_align_poses(T12.ctypes.data, kp.ctypes.data, kp.shape[0], out.ctypes.data)
    if rc != 0:
        raise AlegoError(f"alego_map_align_poses failed ({rc})")
    return out


def _hyp_struct(x, d):
    """fills the MapAlignHyp x from a hypothesis dict of Handle.map_align"""
    for k in ("src_frame", "dst_frame", "dist", "shift", "tried", "accepted", "converged", "iterations", "n_source", "n_target", "support", "inlier"):
        setattr(x, k, int(d[k]))
    x.fitness = float(d["fitness"])
    x.guess6[:] = np.asarray(d["guess6"], np.float32).reshape(6).tolist()
    x.icp_final[:] = np.asarray(d["icp_final"], np.float32).reshape(16).tolist()
    x.T[:] = np.asarray(d["T"], np.float32).reshape(16).tolist()


def map_align_edge(hyp, dst_pose6, nd):
    """alego_map_align_edge: the cross edge (dict frm, to, between (3, 4), variance (6,)) of one accepted inlier hypothesis of Handle.map_align for a
    destination of nd frames whose key pose of hyp["dst_frame"] is dst_pose6 (host code of the library)"""
    x = MapAlignHyp()
    _hyp_struct(x, hyp)
    kp = np.ascontiguousarray(dst_pose6, np.float32).reshape(6)
    e = (GraphEdge * 1)()
    rc = lib().alego_map_align_edge(C.byref(x), kp.ctypes.data, int(nd), e)
    if rc != 0:
        raise AlegoError(f"alego_map_align_edge failed ({rc})")
    g = _graph_edges_out(e, 1)
    return dict(frm=int(g["frm"][0]), to=int(g["to"][0]), between=g["between"][0], variance=g["variance"][0])


def map_merge_edges(src_chain, src_loops, nd, prev_pose6, first_pose6, seam_variance):
    """alego_map_merge_edges: (chain, loops) as graph_get_edges dicts - the graph part of a merge behind nd destination frames from the source's chain and
    loop edges (dicts of graph_get_edges), the destination's key pose nd - 1, the first moved pose and the seam's variances (host code of the library)"""
    ns, nl = len(np.asarray(src_chain["frm"]).reshape(-1)), len(np.asarray(src_loops["frm"]).reshape(-1))
    ch = graph_edges(src_chain["frm"], src_chain["to"], src_chain["between"], src_chain["variance"])
    lp = graph_edges(src_loops["frm"], src_loops["to"], src_loops["between"], src_loops["variance"])
    a = np.ascontiguousarray(np.zeros(6) if prev_pose6 is None else prev_pose6, np.float32).reshape(6)
    b = np.ascontiguousarray(first_pose6, np.float32).reshape(6)
    v = np.ascontiguousarray(seam_variance, np.float64).reshape(6)
    oc, ol = (GraphEdge * max(ns, 1))(), (GraphEdge * max(nl, 1))()
    rc = lib().alego_map_merge_edges(ch, ns, lp, nl, int(nd), a.ctypes.data, b.ctypes.data, v.ctypes.data, oc, ol)
    if rc != 0:
        raise AlegoError(f"alego_map_merge_edges failed ({rc})")
    return _graph_edges_out(oc, ns), _graph_edges_out(ol, nl)


def _thin_arrays(keyposes6, protect):
    kp = np.ascontiguousarray(keyposes6, np.float32).reshape(-1, 6)
    pr = np.zeros(kp.shape[0], np.uint8) if protect is None else np.ascontiguousarray(np.asarray(protect) != 0, np.uint8).reshape(-1)
    if pr.shape[0] != kp.shape[0]:
        raise ValueError("protect: one byte per frame")
    return kp, pr, np.zeros(max(kp.shape[0], 1), np.uint8)


def map_thin_select(keyposes6, protect, min_dist):
    """alego_map_thin_select: the keep mask (n,) uint8 of alego_map_thin's selection rule for key poses (n, 6) and a protect mask (host code of the library)"""
    kp, pr, keep = _thin_arrays(keyposes6, protect)
    rc = lib().alego_map_thin_select(kp.ctypes.data, pr.ctypes.data, kp.shape[0], float(min_dist), keep.ctypes.data)
    if rc < 0:
        raise AlegoError(f"alego_map_thin_select failed ({rc})")
    assert rc == int(keep[:kp.shape[0]].sum())
    return keep[:kp.shape[0]]


def map_thin_edges(chain, loops, keep):
    """alego_map_thin_edges: (chain, loops) as graph_get_edges dicts - the graph of the kept frames from a slot's chain and loop edges (dicts of
    graph_get_edges) and a keep mask (host code of the library)"""
    n, nl = len(np.asarray(chain["frm"]).reshape(-1)), len(np.asarray(loops["frm"]).reshape(-1))
    ch = graph_edges(chain["frm"], chain["to"], chain["between"], chain["variance"])
    lp = graph_edges(loops["frm"], loops["to"], loops["between"], loops["variance"])
    k = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).reshape(-1)
    if k.shape[0] != n:
        raise ValueError("keep: one byte per chain edge")
    oc, ol = (GraphEdge * max(n, 1))(), (GraphEdge * max(nl, 1))()
    rc = lib().alego_map_thin_edges(ch, n, lp, nl, k.ctypes.data, oc, ol)
    if rc < 0:
        raise AlegoError(f"alego_map_thin_edges failed ({rc})")
    return _graph_edges_out(oc, rc), _graph_edges_out(ol, nl)


def occ_opts(origin, cell, n, min_range=0.0, max_range=0.0):
    """alego_occ_opts: origin (3,), cell (3,) or one edge length, n (3,) cells per axis"""
    c = np.broadcast_to(np.asarray(cell, np.float64), (3,))
    return OccOpts((C.c_double * 3)(*[float(v) for v in origin]), (C.c_double * 3)(*[float(v) for v in c]), (C.c_int32 * 3)(*[int(v) for v in n]), 0,
                   float(min_range), float(max_range))


def _occ_rule(rule):
    return None if rule is None else C.byref(OccRule(int(rule[0]), int(rule[1]), int(rule[2]), 0))


def _occ_shape(opts, collapse_z=False):
    return (int(opts.n[1]), int(opts.n[0])) if collapse_z else (int(opts.n[2]), int(opts.n[1]), int(opts.n[0]))


def occ_ray_host(opts, o, e, cap=None):
    """alego_occ_ray_host: (cells (m, 3) int32, hit) of the ray o -> e (f32), or (skip code, None) for a ray that is skipped (host code of the library)"""
    o, e = np.ascontiguousarray(o, np.float32).reshape(3), np.ascontiguousarray(e, np.float32).reshape(3)
    hit = C.c_int32(0)
    if cap is None:
        cap = lib().alego_occ_ray_host(C.byref(opts), o.ctypes.data, e.ctypes.data, None, 0, C.byref(hit))
        if cap < 0:
            if cap == ERR_ARG:
                raise AlegoError("alego_occ_ray_host failed (-4)")
            return cap, None
    cells = np.zeros((max(cap, 1), 3), np.int32)
    n = lib().alego_occ_ray_host(C.byref(opts), o.ctypes.data, e.ctypes.data, cells.ctypes.data, cap, C.byref(hit))
    if n == ERR_ARG:
        raise AlegoError("alego_occ_ray_host failed (-4)")
    return (n, None) if n < 0 else (cells[:min(n, cap)].copy(), int(hit.value))


def occ_integrate_host(opts, origins, pts, hits=None, passes=None, stats=None):
    """alego_occ_integrate_host: (hits, passes, stats) after the points (n, 4) (w = frame id) are cast from origins (frames, 4); given arrays are added to"""
    shape = _occ_shape(opts)
    hits = np.zeros(shape, np.uint32) if hits is None else hits
    passes = np.zeros(shape, np.uint32) if passes is None else passes
    stats = np.zeros(OCC_STATS, np.int64) if stats is None else stats
    kp, p = np.ascontiguousarray(origins, np.float32).reshape(-1, 4), np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    assert hits.flags.c_contiguous and passes.flags.c_contiguous and hits.dtype == np.uint32 and passes.dtype == np.uint32 and stats.dtype == np.int64
    if p.shape[0] and (p[:, 3].min() < 0 or p[:, 3].max() >= kp.shape[0]):
        raise ValueError("a point names a frame without an origin")
    rc = lib().alego_occ_integrate_host(C.byref(opts), kp.ctypes.data, p.ctypes.data, p.shape[0], hits.ctypes.data, passes.ctypes.data, stats.ctypes.data)
    if rc < 0:
        raise AlegoError(f"alego_occ_integrate_host failed ({rc})")
    return hits, passes, stats


def occ_classify_host(opts, hits, passes, rule=None, collapse_z=False):
    """alego_occ_classify_host: int8 classes (100 / 0 / -1) of the counts; rule = (min_hits, hit_weight, pass_weight) or None for the defaults"""
    h, p = np.ascontiguousarray(hits, np.uint32), np.ascontiguousarray(passes, np.uint32)
    out = np.zeros(_occ_shape(opts, collapse_z), np.int8)
    rc = lib().alego_occ_classify_host(C.byref(opts), _occ_rule(rule), h.ctypes.data, p.ctypes.data, int(bool(collapse_z)), out.ctypes.data)
    if rc < 0:
        raise AlegoError(f"alego_occ_classify_host failed ({rc})")
    return out


def static_rule(occ=(1, 2, 1), protect_radius=0, keep_below=None):
    """alego_static_rule: occ = (min_hits, hit_weight, pass_weight); keep_below = None leaves that test off"""
    return StaticRule(OccRule(int(occ[0]), int(occ[1]), int(occ[2]), 0), int(protect_radius), 0 if keep_below is None else 1,
                      0.0 if keep_below is None else float(keep_below), 0)


def _static_rule(rule):
    return None if rule is None else C.byref(rule)


def occ_mark_host(opts, hits, passes, pts, rule=None, sensor_z=None):
    """alego_occ_mark_host: (verdicts (n,) uint8, stats (STATIC_VERDICTS,) int64) of the world points (n, 3+) against the counts; rule from static_rule() or
    None for the defaults; sensor_z (n,) f32 is needed when the rule has keep_below"""
    h, p = np.ascontiguousarray(hits, np.uint32), np.ascontiguousarray(passes, np.uint32)
    assert h.size == p.size == int(opts.n[0]) * int(opts.n[1]) * int(opts.n[2])
    a = np.asarray(pts, np.float32)
    q = np.zeros((a.shape[0], 4), np.float32)
    q[:, :3] = a[:, :3]
    z = None if sensor_z is None else np.ascontiguousarray(sensor_z, np.float32).reshape(q.shape[0])
    verdict, stats = np.zeros(max(q.shape[0], 1), np.uint8), np.zeros(STATIC_VERDICTS, np.int64)
    rc = lib().alego_occ_mark_host(C.byref(opts), _static_rule(rule), h.ctypes.data, p.ctypes.data, q.ctypes.data, None if z is None else z.ctypes.data, q.shape[0],
                                   verdict.ctypes.data, stats.ctypes.data)
    if rc < 0:
        raise AlegoError(f"alego_occ_mark_host failed ({rc})")
    return verdict[:q.shape[0]], stats


def occ_inflation(inscribed_radius, inflation_radius, cost_scaling=10.0, inflate_unknown=False):
    """alego_occ_inflation: costmap_2d's inflation parameters, in metres"""
    return OccInflation(float(inscribed_radius), float(inflation_radius), float(cost_scaling), int(bool(inflate_unknown)), 0)


def occ_distance_host(cls, unknown_is_obstacle=False, max_cells=0):
    """alego_occ_distance_host: (d2 uint32 of cls's shape, stats (EDT_STATS,) int64) of a class array (n2, n1, n0), (n1, n0) or (n0,) as occ_classify gives it"""
    c = np.ascontiguousarray(cls, np.int8)
    n = (C.c_int32 * 3)(*([1] * (3 - c.ndim) + list(c.shape))[::-1])
    d2, stats = np.zeros(c.shape, np.uint32), np.zeros(EDT_STATS, np.int64)
    rc = lib().alego_occ_distance_host(c.ctypes.data, n, int(bool(unknown_is_obstacle)), int(max_cells), d2.ctypes.data, stats.ctypes.data)
    if rc < 0:
        raise AlegoError(f"alego_occ_distance_host failed ({rc})")
    return d2, stats


def occ_cost_table_host(s, inflation):
    """alego_occ_cost_table_host: the cost table (r r + 1,) uint8 over d2 for cells of edge s"""
    table = np.empty(4095 * 4095 + 1, np.uint8)   # the largest table there is; the library returns how much of it the parameters use (r r + 1)
    rc = lib().alego_occ_cost_table_host(float(s), C.byref(inflation), table.ctypes.data, table.size)
    if rc < 0:
        raise AlegoError(f"alego_occ_cost_table_host failed ({rc})")
    return table[:rc].copy()


def occ_costmap_host(cls, d2, table, unknown_is_obstacle=False, inflate_unknown=False):
    """alego_occ_costmap_host: the costs uint8 of cls's shape from the classes, their d2 and the cost table"""
    c, d, t = np.ascontiguousarray(cls, np.int8), np.ascontiguousarray(d2, np.uint32), np.ascontiguousarray(table, np.uint8)
    assert c.shape == d.shape
    out = np.zeros(c.shape, np.uint8)
    rc = lib().alego_occ_costmap_host(c.ctypes.data, d.ctypes.data, c.size, int(bool(unknown_is_obstacle)), t.ctypes.data, t.size, int(bool(inflate_unknown)), out.ctypes.data)
    if rc < 0:
        raise AlegoError(f"alego_occ_costmap_host failed ({rc})")
    return out


def _reloc_result(r):
    n = int(r.n_cand)
    return dict(status=int(r.status), n_cand=n, cand_id=np.array(r.cand_id[:n], np.int32), cand_dist=np.array(r.cand_dist[:n], np.int32),
                cand_shift=np.array(r.cand_shift[:n], np.int32), verified=int(r.verified), converged=int(r.converged), iterations=int(r.iterations),
                n_source=int(r.n_source), n_target=int(r.n_target), applied=int(r.applied), fitness=float(r.fitness),
                T=np.array(r.correction[:], np.float32).reshape(4, 4), guess6=np.array(r.guess6[:], np.float32),
                t_map=np.array(r.t_map[:], np.float32).reshape(4, 4), rc=np.array(r.rc[:], np.float64), params6=np.array(r.params6[:], np.float64))


def loop_constraint(correction, latest_pose6, closest_pose6):
    """:714-730 on the host: (t_correct 4x4 f32, between 3x4 f64 [R | t]) from an ICP correction and the newest / closest key poses"""
    c = np.ascontiguousarray(correction, np.float32).reshape(16)
    a = np.ascontiguousarray(latest_pose6, np.float32).reshape(6)
    b = np.ascontiguousarray(closest_pose6, np.float32).reshape(6)
    t = np.zeros(16, np.float32)
    bt = np.zeros(12, np.float64)
    rc = lib().alego_loop_constraint(c.ctypes.data, a.ctypes.data, b.ctypes.data, t.ctypes.data, bt.ctypes.data)
    if rc != 0:
        raise AlegoError(f"alego_loop_constraint failed ({rc})")
    return t.reshape(4, 4), bt.reshape(3, 4)


def pc2_to_points(data: bytes, width, height, point_step, row_step, fields, is_bigendian=False, cap=None):
    """sensor_msgs/PointCloud2 payload -> (n, 4) float32 (x, y, z, intensity); fields = [(name, offset, datatype, count), ...].
    Host-side (no GPU needed): the ROS-free equivalent of pcl::fromROSMsg<PointXYZI> in front of alego_ip_process."""
    n = width * height
    cap = n if cap is None else cap
    out = np.empty((max(cap, 1), 4), np.float32)
    arr = (Pc2Field * len(fields))(*[Pc2Field(nm.encode(), off, dt, cnt) for nm, off, dt, cnt in fields])
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data) if len(data) else None
    rc = lib().alego_pc2_to_points(buf, len(data), width, height, point_step, row_step, 1 if is_bigendian else 0, arr, len(fields),
                                   out.ctypes.data, cap)
    if rc < 0:
        raise AlegoError(f"alego_pc2_to_points failed ({rc})")
    return out[:rc].copy()


class Bag:
    """A rosbag format 2.0 file opened by the library's own reader (no ROS): topics, and the PointCloud2 messages of a topic in
    time order — what `rosbag play` + the /lslidar_point_cloud subscriber + pcl::fromROSMsg deliver to ImageProjection."""

    def __init__(self, path):
        h = C.c_void_p()
        rc = lib().alego_bag_open(os.fsencode(path), C.byref(h))
        if rc != 0:
            raise AlegoError(f"alego_bag_open({path}) failed ({rc}): not a readable rosbag 2.0 file (see stderr)")
        self._b = h

    def close(self):
        if getattr(self, "_b", None):
            lib().alego_bag_close(self._b)
            self._b = None

    def __del__(self):
        self.close()

    def _err(self):
        return lib().alego_bag_last_error(self._b).decode(errors="replace")

    def topics(self):
        """{topic: (datatype, number of messages)}"""
        out = {}
        for i in range(lib().alego_bag_topic_count(self._b)):
            t, d, n = C.c_char_p(), C.c_char_p(), C.c_int64()
            lib().alego_bag_topic_info(self._b, i, C.byref(t), C.byref(d), C.byref(n))
            out[t.value.decode()] = (d.value.decode(), int(n.value))
        return out

    def message_count(self, topic):
        return int(lib().alego_bag_message_count(self._b, topic.encode()))

    def read_raw(self, topic, index):
        """(serialized message bytes, bag time)"""
        p, n, t = C.c_void_p(), C.c_uint64(), C.c_double()
        rc = lib().alego_bag_read_raw(self._b, topic.encode(), index, C.byref(p), C.byref(n), C.byref(t))
        if rc != 0:
            raise AlegoError(f"alego_bag_read_raw failed ({rc}): {self._err()}")
        return C.string_at(p.value, n.value), float(t.value)

    def read_pc2(self, topic, index, cap=1 << 20):
        """(points[n, 4] float32, header stamp, is_dense)"""
        out = np.empty((cap, 4), np.float32)
        st, dn = C.c_double(), C.c_int32()
        n = lib().alego_bag_read_pc2(self._b, topic.encode(), index, out.ctypes.data, cap, C.byref(st), C.byref(dn))
        if n < 0:
            raise AlegoError(f"alego_bag_read_pc2 failed ({n}): {self._err()}")
        return out[:n].copy(), float(st.value), bool(dn.value)


_CLOUDS = {"seg_cloud", "undistorted", "outlier", "sharp", "less_sharp", "flat", "less_flat"}


class Handle:
    """One alego_handle: `n_slots` independent streams advanced in lock-step on one GPU."""

    def __init__(self, params: AlegoParams, device: int = 0, n_slots: int = 1, ring_len: int = 1):
        L = lib()
        self.params = params
        self.N = params.n_scan * params.horizon_scan
        self.n_slots, self.ring_len = n_slots, ring_len
        h = C.c_void_p()
        rc = L.alego_create(C.byref(params), device, n_slots, ring_len, C.byref(h))
        if rc != 0:
            why = {-1: "no gfx950 device (there is no CPU fallback)", -2: "a HIP call failed", -3: "capacity", -4: "a parameter is outside the supported range (see stderr)"}.get(rc, "?")
            raise AlegoError(f"alego_create failed ({rc}): {why}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            bad, rep = check_guards()   # (ALEGO_DEBUG_CANARY=1: did a kernel write outside a buffer?  -1 = not enabled)
            lib().alego_destroy(self._h)
            self._h = None
            if bad > 0:
                raise AlegoError(f"device memory guards damaged: {rep}")

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise AlegoError(f"{what} failed ({rc}): {lib().alego_last_error(self._h).decode()}")
        return rc

    # ---- buffers ----
    def _seg_bufs(self, want_labels):
        N, NS = self.N, self.params.n_scan
        b = dict(seg=np.empty((N, 4), np.float32), ground=np.empty(N, np.uint8), col=np.empty(N, np.int32),
                 range=np.empty(N, np.float32), ring_start=np.empty(NS, np.int32), ring_end=np.empty(NS, np.int32),
                 outlier=np.empty((N, 4), np.float32), label_image=np.empty(N, np.int32) if want_labels else None)
        s = SegOut()
        s.seg, s.seg_cap = b["seg"].ctypes.data, N
        s.ground, s.col, s.range = b["ground"].ctypes.data, b["col"].ctypes.data, b["range"].ctypes.data
        s.ring_start, s.ring_end = b["ring_start"].ctypes.data, b["ring_end"].ctypes.data
        s.outlier, s.outlier_cap = b["outlier"].ctypes.data, N
        s.label_image = b["label_image"].ctypes.data if want_labels else None
        return s, b

    @staticmethod
    def _seg_result(s, b):
        m, no = s.m, s.n_outlier
        return dict(seg=b["seg"][:m].copy(), ground=b["ground"][:m].copy(), col=b["col"][:m].copy(), range=b["range"][:m].copy(),
                    ring_start=b["ring_start"].copy(), ring_end=b["ring_end"].copy(), orientation=np.array(s.orientation[:], np.float32),
                    outlier=b["outlier"][:no].copy(), label_image=None if b["label_image"] is None else b["label_image"].copy())

    def _feat_bufs(self, want_labels=True):
        N = self.N
        caps = (N, N, N, N)
        b = dict(sharp=np.empty((caps[0], 4), np.float32), less_sharp=np.empty((caps[1], 4), np.float32),
                 flat=np.empty((caps[2], 4), np.float32), less_flat=np.empty((caps[3], 4), np.float32),
                 point_label=np.empty(N, np.int32) if want_labels else None)
        f = FeatOut()
        f.sharp, f.sharp_cap = b["sharp"].ctypes.data, caps[0]
        f.less_sharp, f.less_sharp_cap = b["less_sharp"].ctypes.data, caps[1]
        f.flat, f.flat_cap = b["flat"].ctypes.data, caps[2]
        f.less_flat, f.less_flat_cap = b["less_flat"].ctypes.data, caps[3]
        f.point_label = b["point_label"].ctypes.data if want_labels else None
        return f, b

    @staticmethod
    def _feat_result(f, b, m=None):
        return dict(sharp=b["sharp"][:f.n_sharp].copy(), less_sharp=b["less_sharp"][:f.n_less_sharp].copy(),
                    flat=b["flat"][:f.n_flat].copy(), less_flat=b["less_flat"][:f.n_less_flat].copy(),
                    point_label=None if b["point_label"] is None else (b["point_label"][:m].copy() if m is not None else b["point_label"].copy()))

    @staticmethod
    def _scan(pts, stamp=0.0):
        a = np.ascontiguousarray(pts, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] == 4
        s = ScanIn()
        s.pts, s.n, s.stamp = a.ctypes.data, a.shape[0], float(stamp)
        return s, a

    # ---- nodelet-shaped entry points ----
    def ip_process(self, pts, want_labels=True, stamp=0.0):
        sin, keep = self._scan(pts, stamp)
        s, b = self._seg_bufs(want_labels)
        self._check(lib().alego_ip_process(self._h, C.byref(sin), C.byref(s)), "alego_ip_process")
        r = self._seg_result(s, b)
        r["stamp"] = s.stamp
        return r

    def lo_process(self, seg):
        """seg: dict as returned by ip_process (what LO receives on /segmented_cloud + /seg_info)."""
        m = seg["seg"].shape[0]
        s = SegOut()
        arrs = [np.ascontiguousarray(seg["seg"], np.float32), np.ascontiguousarray(seg["ground"], np.uint8),
                np.ascontiguousarray(seg["col"], np.int32), np.ascontiguousarray(seg["range"], np.float32),
                np.ascontiguousarray(seg["ring_start"], np.int32), np.ascontiguousarray(seg["ring_end"], np.int32)]
        s.seg, s.seg_cap, s.m = arrs[0].ctypes.data, m, m
        s.ground, s.col, s.range = arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data
        s.ring_start, s.ring_end = arrs[4].ctypes.data, arrs[5].ctypes.data
        if "orientation" in seg:
            s.orientation[:] = [float(v) for v in seg["orientation"]]
        s.stamp = float(seg.get("stamp", 0.0))
        f, fb = self._feat_bufs()
        odom = Pose()
        flags = self._check(lib().alego_lo_process(self._h, C.byref(s), C.byref(f), C.byref(odom)), "alego_lo_process")
        return flags, self._feat_result(f, fb, m), odom.as_dict()

    def lm_process(self, corner_last, surf_last, outlier, odom):
        c = np.ascontiguousarray(corner_last, np.float32)
        s = np.ascontiguousarray(surf_last, np.float32)
        o = np.ascontiguousarray(outlier, np.float32)
        po, pm = Pose(), Pose()
        po.t[:] = list(odom["t"]); po.q[:] = list(odom["q"]); po.valid = 1
        flags = self._check(lib().alego_lm_process(self._h, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0],
                                                    o.ctypes.data, o.shape[0], C.byref(po), C.byref(pm)), "alego_lm_process")
        return flags, pm.as_dict()

    def scan_process(self, pts, stages=7, slot=0, want_outputs=False, stamp=0.0):
        sin, keep = self._scan(pts, stamp)
        odom, mp = Pose(), Pose()
        if want_outputs:
            s, b = self._seg_bufs(True)
            f, fb = self._feat_bufs()
            flags = self._check(lib().alego_scan_process(self._h, slot, C.byref(sin), stages, C.byref(s), C.byref(f),
                                                          C.byref(odom), C.byref(mp)), "alego_scan_process")
            return flags, odom.as_dict(), mp.as_dict(), self._seg_result(s, b), self._feat_result(f, fb, s.m)
        flags = self._check(lib().alego_scan_process(self._h, slot, C.byref(sin), stages, None, None, C.byref(odom), C.byref(mp)),
                            "alego_scan_process")
        return flags, odom.as_dict(), mp.as_dict()

    # ---- batch path ----
    def batch_load(self, slot, ring_pos, pts):
        a = np.ascontiguousarray(pts, dtype=np.float32)
        self._check(lib().alego_batch_load(self._h, slot, ring_pos, a.ctypes.data, a.shape[0]), "alego_batch_load")

    def replay_create(self, n_bags, bag_len):
        self._check(lib().alego_replay_create(self._h, n_bags, bag_len), "alego_replay_create")

    def replay_load(self, bag, scan, pts):
        a = np.ascontiguousarray(pts, dtype=np.float32)
        self._check(lib().alego_replay_load(self._h, bag, scan, a.ctypes.data, a.shape[0]), "alego_replay_load")

    def replay_assign(self, slot, bag, start_scan):
        self._check(lib().alego_replay_assign(self._h, slot, bag, start_scan), "alego_replay_assign")

    def stream_setup(self, bag, start_scan=0):
        """slot 0 = one stream replaying `bag`; the other slots become its look-ahead lanes (alego_stream_run)"""
        self._check(lib().alego_stream_setup(self._h, bag, start_scan), "alego_stream_setup")

    def stream_run(self, first_step, n_scans, stages=7, sync=True):
        self._check(lib().alego_stream_run(self._h, first_step, n_scans, stages, 1 if sync else 0), "alego_stream_run")

    def batch_run(self, first_pos, n_scans, stages=7, sync=True):
        self._check(lib().alego_batch_run(self._h, first_pos, n_scans, stages, 1 if sync else 0), "alego_batch_run")

    def synchronize(self):
        self._check(lib().alego_synchronize(self._h), "alego_synchronize")

    def batch_get_pose(self, slot=0):
        odom, mp = Pose(), Pose()
        flags = self._check(lib().alego_batch_get_pose(self._h, slot, C.byref(odom), C.byref(mp)), "alego_batch_get_pose")
        return flags, odom.as_dict(), mp.as_dict()

    def batch_get_counts(self, slot=0):
        out = np.zeros(16, np.int32)
        self._check(lib().alego_batch_get_counts(self._h, slot, out.ctypes.data, 16), "alego_batch_get_counts")
        keys = ["P", "M", "O", "Qc", "Fc", "Qs", "Fs", "n_surf_corr", "n_corner_corr", "Kraw_c", "Kraw_s", "Kds_c", "Kds_s", "Lc", "Ls", "n_rebuild"]
        return dict(zip(keys, out.tolist()))

    def profile_enable(self, on=True):
        self._check(lib().alego_profile_enable(self._h, 1 if on else 0), "alego_profile_enable")

    def profile_report(self):
        """{kernel name: (total ms, launches)} measured with HIP events on the handle's stream."""
        names = C.create_string_buffer(8192)
        tot = np.zeros(256, np.float64)
        cnt = np.zeros(256, np.int32)
        n = self._check(lib().alego_profile_report(self._h, names, 8192, tot.ctypes.data, cnt.ctypes.data, 256), "alego_profile_report")
        ks = names.value.decode().split(";") if n else []
        return {k: (float(tot[i]), int(cnt[i])) for i, k in enumerate(ks)}

    def stream(self):
        return lib().alego_stream(self._h)

    def stream_groups(self):
        """(number of HIP stream groups, slots covered by one kernel launch)"""
        per = C.c_int(0)
        g = lib().alego_stream_groups(self._h, C.byref(per))
        return g, per.value

    def stream_plan(self):
        """alego_stream_plan: dict(groups, slots_per_group, lm_async, hw_queues) — the streams the handle drives and the queue count they were fitted to"""
        out = (C.c_int * 4)()
        self._check(lib().alego_stream_plan(self._h, out), "alego_stream_plan")
        return dict(groups=out[0], slots_per_group=out[1], lm_async=bool(out[2]), hw_queues=out[3])

    # ---- test access ----
    def set_lo_params(self, p6, slot=0):
        a = np.ascontiguousarray(p6, np.float64)
        self._check(lib().alego_set_lo_params(self._h, slot, a.ctypes.data), "alego_set_lo_params")

    def set_lm_params(self, p6, slot=0):
        a = np.ascontiguousarray(p6, np.float64)
        self._check(lib().alego_set_lm_params(self._h, slot, a.ctypes.data), "alego_set_lm_params")

    def debug_get(self, name, slot=0, cap_bytes=None):
        cap = cap_bytes or max(self.N * 64 + 4096, 8 << 20)
        buf = np.empty(cap, np.uint8)
        cnt, dt = C.c_int(), C.c_int()
        self._check(lib().alego_debug_get(self._h, slot, name.encode(), buf.ctypes.data, cap, C.byref(cnt), C.byref(dt)),
                    f"alego_debug_get({name})")
        dtype = np.dtype(_DT[dt.value])
        out = np.frombuffer(buf.tobytes()[:cnt.value * dtype.itemsize], dtype=dtype).copy()
        return out.reshape(-1, 4) if (name in _CLOUDS or name.startswith("lm_") and name.endswith(("_ds", "_map"))) else out

    def voxel_grid(self, pts, leaf):
        """The device VoxelGrid on a host cloud (debug entry; both the LDS path and the bucket-sort path)."""
        a = np.ascontiguousarray(pts, np.float32)
        out = np.empty((max(a.shape[0], 1), 4), np.float32)
        n = self._check(lib().alego_debug_voxel(self._h, a.ctypes.data, a.shape[0], leaf, out.ctypes.data, out.shape[0]), "alego_debug_voxel")
        return out[:n].copy()

    def voxel_grid_large(self, pts, leaf):
        """alego_voxel_grid: pcl::VoxelGrid of a host cloud of any size (the product entry point; large clouds on the whole device)"""
        a = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        n = self._check(lib().alego_voxel_grid(self._h, a.ctypes.data, a.shape[0], leaf, None, 0), "alego_voxel_grid")
        out = np.empty((max(n, 1), 4), np.float32)
        m = self._check(lib().alego_voxel_grid(self._h, a.ctypes.data, a.shape[0], leaf, out.ctypes.data, out.shape[0]), "alego_voxel_grid")
        return out[:m].copy()

    # ---- the global map (key-frame archive) ----
    def map_enable(self, max_keyframes, max_points):
        self._check(lib().alego_map_enable(self._h, max_keyframes, max_points), "alego_map_enable")

    def map_status(self, slot=0):
        """(frames stored, frames dropped, points stored, point capacity)"""
        out = np.zeros(4, np.int32)
        self._check(lib().alego_map_status(self._h, slot, out.ctypes.data), "alego_map_status")
        return tuple(int(v) for v in out)

    def map_set_keyposes(self, first, poses6, slot=0):
        a = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
        self._check(lib().alego_map_set_keyposes(self._h, slot, first, a.shape[0], a.ctypes.data), "alego_map_set_keyposes")

    def map_get_keyframe(self, kf_id, slot=0):
        """dict(id, pose[6], corner, surf, outlier): any archived key frame"""
        k = KeyFrame()
        self._check(lib().alego_map_get_keyframe(self._h, slot, kf_id, C.byref(k)), "alego_map_get_keyframe")   # (counts only)
        bufs = [np.empty((max(n, 1), 4), np.float32) for n in (k.n_corner, k.n_surf, k.n_outlier)]
        k.corner, k.corner_cap = bufs[0].ctypes.data, bufs[0].shape[0]
        k.surf, k.surf_cap = bufs[1].ctypes.data, bufs[1].shape[0]
        k.outlier, k.outlier_cap = bufs[2].ctypes.data, bufs[2].shape[0]
        self._check(lib().alego_map_get_keyframe(self._h, slot, kf_id, C.byref(k)), "alego_map_get_keyframe")
        return dict(id=int(k.id), pose=np.array(k.pose[:], np.float32), corner=bufs[0][:k.n_corner].copy(), surf=bufs[1][:k.n_surf].copy(),
                    outlier=bufs[2][:k.n_outlier].copy())

    def map_assemble(self, kinds, leaf=0.0, slot=0, cap=None):
        """the global map of `slot` (ALEGO_MAP_* kinds, optionally VoxelGrid(leaf)); cap: output capacity (default: the count)"""
        if cap is None:
            cap = self._check(lib().alego_map_assemble(self._h, slot, kinds, leaf, None, 0), "alego_map_assemble")
        out = np.empty((max(cap, 1), 4), np.float32)
        n = self._check(lib().alego_map_assemble(self._h, slot, kinds, leaf, out.ctypes.data, cap), "alego_map_assemble")
        return out[:n].copy()

    def map_get_stamps(self, first=0, n=None, slot=0):
        if n is None:
            n = self.map_status(slot)[0] - first
        out = np.zeros(max(n, 1), np.float64)
        self._check(lib().alego_map_get_stamps(self._h, slot, first, n, out.ctypes.data), "alego_map_get_stamps")
        return out[:n].copy()

    def map_set_stamps(self, first, stamps, slot=0):
        a = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        self._check(lib().alego_map_set_stamps(self._h, slot, first, a.shape[0], a.ctypes.data), "alego_map_set_stamps")

    def map_keyposes(self, slot=0):
        n = self._check(lib().alego_map_keyposes(self._h, slot, None, 0), "alego_map_keyposes")
        out = np.empty((max(n, 1), 4), np.float32)
        n = self._check(lib().alego_map_keyposes(self._h, slot, out.ctypes.data, out.shape[0]), "alego_map_keyposes")
        return out[:n].copy()

    def lm_local_map(self, slot=0):
        """(corner_from_map_ds_, surf_from_map_ds_) of the last mapping frame"""
        n = np.zeros(2, np.int32)
        self._check(lib().alego_lm_get_local_map(self._h, slot, None, 0, None, 0, n.ctypes.data), "alego_lm_get_local_map")
        c, s = np.empty((max(int(n[0]), 1), 4), np.float32), np.empty((max(int(n[1]), 1), 4), np.float32)
        self._check(lib().alego_lm_get_local_map(self._h, slot, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], n.ctypes.data), "alego_lm_get_local_map")
        return c[:n[0]].copy(), s[:n[1]].copy()

    def math(self, mode, a, b=None):
        """device single-precision functions: mode 0 atan2f(a, b), 1 hypotf(a, b), 2 sinf(a), 3 cosf(a)"""
        a = np.ascontiguousarray(a, np.float32)
        b = None if b is None else np.ascontiguousarray(b, np.float32)
        out = np.empty_like(a)
        self._check(lib().alego_debug_math(self._h, mode, a.ctypes.data, None if b is None else b.ctypes.data, out.ctypes.data, a.size), "alego_debug_math")
        return out

    def trajectory_enable(self, capacity):
        self._check(lib().alego_trajectory_enable(self._h, capacity), "alego_trajectory_enable")
        self._traj_cap = capacity

    def trajectory(self, slot=0, first=0, n=None):
        """poses[n, 14] logged for `slot`: odom t(3) q(4), map t(3) q(4) per processed scan"""
        if n is None:
            n = min(self._check(lib().alego_trajectory_get(self._h, slot, 0, 0, None), "alego_trajectory_get"), self._traj_cap) - first
        out = np.empty((max(n, 0), 14), np.float64)
        self._check(lib().alego_trajectory_get(self._h, slot, first, max(n, 0), out.ctypes.data), "alego_trajectory_get")
        return out

    def undistorted(self, slot=0):
        """/undistorted: the de-skewed segmented cloud of the slot's last scan (deskew_mode = 1), [M, 4] f32"""
        out = np.zeros((self.N, 4), np.float32)
        n = self._check(lib().alego_lo_get_undistorted(self._h, slot, out.ctypes.data, out.shape[0]), "alego_lo_get_undistorted")
        return out[:n].copy()

    def push_imu(self, samples, slot=0):
        """samples[n, 11]: stamp, orientation w x y z, linear_acceleration xyz, angular_velocity xyz (sensor_msgs/Imu)"""
        a = np.ascontiguousarray(samples, np.float64).reshape(-1, 11)
        self._check(lib().alego_lo_push_imu(self._h, slot, a.ctypes.data, a.shape[0]), "alego_lo_push_imu")

    def std_sort(self, keys, depth_limit=-1):
        """index order libstdc++'s std::sort gives 0..n-1 under `keys[a] < keys[b]`, as the device reproduces it (sort_mode 2)"""
        k = np.ascontiguousarray(keys, np.uint32)
        out = np.empty(k.size, np.int32)
        self._check(lib().alego_debug_std_sort(self._h, k.ctypes.data, k.size, depth_limit, out.ctypes.data), "alego_debug_std_sort")
        return out

    def eval_blocks(self, btype, geom13, params6):
        """(residuals[n], jacobians[n, 6]) of cost functor `btype` evaluated on the device as the solvers do"""
        g = np.ascontiguousarray(geom13, np.float64).reshape(-1, 13)
        p = np.ascontiguousarray(params6, np.float64)
        r, J = np.empty(g.shape[0]), np.empty((g.shape[0], 6))
        self._check(lib().alego_debug_eval_blocks(self._h, btype, g.shape[0], g.ctypes.data, p.ctypes.data, r.ctypes.data, J.ctypes.data), "alego_debug_eval_blocks")
        return r, J

    def transform_to_start(self, params6, pts):
        p = np.ascontiguousarray(params6, np.float64)
        a = np.ascontiguousarray(pts, np.float32)
        out = np.empty_like(a)
        self._check(lib().alego_debug_transform_to_start(self._h, p.ctypes.data, a.ctypes.data, a.shape[0], out.ctypes.data), "alego_debug_transform_to_start")
        return out

    def set_option(self, name, value):
        self._check(lib().alego_debug_set_option(self._h, name.encode(), int(value)), f"alego_debug_set_option({name})")

    # ---- loop closure ----
    def loop_closure_icp(self, frames):
        """frames = [(pose6, corner, surf, outlier), ...]: the newest key frame, then the history frames.  Returns (result dict, target cloud)."""
        keep, kfs = [], (KfIn * len(frames))()
        total = 0
        for i, f in enumerate(frames):
            kfs[i].pose[:] = [float(v) for v in f[0]]
            arrs = [np.ascontiguousarray(c, np.float32).reshape(-1, 4) for c in f[1:4]]
            keep.append(arrs)
            kfs[i].corner, kfs[i].n_corner = arrs[0].ctypes.data, arrs[0].shape[0]
            kfs[i].surf, kfs[i].n_surf = arrs[1].ctypes.data, arrs[1].shape[0]
            kfs[i].outlier, kfs[i].n_outlier = arrs[2].ctypes.data, arrs[2].shape[0]
            total += sum(a.shape[0] for a in arrs)
        out = IcpResult()
        tgt = np.empty((max(total, 1), 4), np.float32)
        hist = C.cast(C.byref(kfs, C.sizeof(KfIn)), C.POINTER(KfIn)) if len(frames) > 1 else None
        self._check(lib().alego_loop_closure_icp(self._h, C.byref(kfs[0]), hist, len(frames) - 1, C.byref(out), tgt.ctypes.data, tgt.shape[0]),
                    "alego_loop_closure_icp")
        return dict(converged=int(out.converged), iterations=int(out.iterations), n_source=int(out.n_source), n_target=int(out.n_target),
                    fitness=float(out.fitness), T=np.array(out.correction[:], np.float32).reshape(4, 4)), tgt[:out.n_target].copy()

    def loop_search(self, slots):
        """alego_loop_search: one dict per listed slot (status, ids, converged, iterations, n_source, n_target, fitness, T, t_correct,
        between, noise_variance)"""
        sl, n = _slot_list(slots)
        out = (LoopResult * max(n, 1))()
        self._check(lib().alego_loop_search(self._h, sl.ctypes.data, n, out), "alego_loop_search")
        return [_loop_result(out[i]) for i in range(n)]

    # ---- loop closures by appearance (needs map_enable) ----
    def loop_appearance_enable(self, max_range=0.0, z_offset=float("nan")):
        self._check(lib().alego_loop_appearance_enable(self._h, float(max_range), float(z_offset)), "alego_loop_appearance_enable")

    def loop_search_appearance(self, slots, n_cand=0, verify=-1, max_dist=0, max_jump=0.0, fitness_max=0.0):
        """alego_loop_search_appearance: one dict per listed slot — loop_search's keys (T = the world correction: graph_add_loops takes the dicts
        unchanged) plus n_eligible, n_cand, cand_id, cand_dist, cand_shift, verified, guess6, icp_final"""
        sl, n = _slot_list(slots)
        out = (LoopResult * max(n, 1))()
        info = (LoopAppInfo * max(n, 1))()
        opts = LoopAppOpts(int(n_cand), int(verify), int(max_dist), float(max_jump), float(fitness_max))
        self._check(lib().alego_loop_search_appearance(self._h, sl.ctypes.data, n, C.byref(opts), out, info), "alego_loop_search_appearance")
        res = []
        for i in range(n):
            d, f = _loop_result(out[i]), info[i]
            k = int(f.n_cand)
            d.update(n_eligible=int(f.n_eligible), n_cand=k, cand_id=np.array(f.cand_id[:k], np.int32), cand_dist=np.array(f.cand_dist[:k], np.int32),
                     cand_shift=np.array(f.cand_shift[:k], np.int32), verified=int(f.verified), guess6=np.array(f.guess6[:], np.float32),
                     icp_final=np.array(f.icp_final[:], np.float32).reshape(4, 4))
            res.append(d)
        return res

    # ---- one slot's archive aligned to another's (needs loop_appearance_enable) ----
    def map_align(self, pairs, n_queries=0, n_cand=0, max_dist=0, min_support=0, fitness_max=0.0, tol_trans=0.0, tol_rot=0.0, hyps=True):
        """alego_map_align: one dict per pair (src, dst) — status, n_queries, n_accepted, best, support, T (3, 4) f64 and, with hyps, `hyp`: one dict per
        query (src_frame, dst_frame, dist, shift, tried, accepted, converged, iterations, n_source, n_target, support, inlier, fitness, guess6, icp_final, T)"""
        src, dst, n = _slot_list(pairs, pairs=True)
        out = (MapAlignResult * max(n, 1))()
        hyp = (MapAlignHyp * (max(n, 1) * ALIGN_MAX_QUERIES))() if hyps else None
        opts = MapAlignOpts(int(n_queries), int(n_cand), int(max_dist), int(min_support), float(fitness_max), float(tol_trans), float(tol_rot))
        self._check(lib().alego_map_align(self._h, src.ctypes.data, dst.ctypes.data, n, C.byref(opts), out, hyp), "alego_map_align")
        res = []
        for i in range(n):
            r = out[i]
            d = dict(status=int(r.status), n_queries=int(r.n_queries), n_accepted=int(r.n_accepted), best=int(r.best), support=int(r.support),
                     T=np.array(r.T[:], np.float64).reshape(3, 4))
            if hyps:
                d["hyp"] = []
                for q in range(int(r.n_queries)):
                    x = hyp[i * ALIGN_MAX_QUERIES + q]
                    d["hyp"].append(dict(src_frame=int(x.src_frame), dst_frame=int(x.dst_frame), dist=int(x.dist), shift=int(x.shift), tried=int(x.tried),
                                         accepted=int(x.accepted), converged=int(x.converged), iterations=int(x.iterations), n_source=int(x.n_source),
                                         n_target=int(x.n_target), support=int(x.support), inlier=int(x.inlier), fitness=float(x.fitness),
                                         guess6=np.array(x.guess6[:], np.float32), icp_final=np.array(x.icp_final[:], np.float32).reshape(4, 4),
                                         T=np.array(x.T[:], np.float32).reshape(4, 4)))
            res.append(d)
        return res

    # ---- a slot moved, one slot's archive appended to another's, on the device (needs map_enable) ----
    def map_move(self, slots, T):
        """alego_map_move: T (n, 3, 4) or one (3, 4) / (4, 4) for every listed slot; returns the status per slot (2 moved, 0 no key frame, -1 dropped frames)"""
        sl, n = _slot_list(slots)
        T = np.asarray(T, np.float64)
        if T.ndim == 2:
            T = np.broadcast_to(T, (n,) + T.shape)
        T12 = np.ascontiguousarray(T.reshape(n, T.shape[-2] * T.shape[-1])[:, :12])
        st = np.zeros(max(n, 1), np.int32)
        self._check(lib().alego_map_move(self._h, sl.ctypes.data, n, T12.ctypes.data, st.ctypes.data), "alego_map_move")
        return [int(v) for v in st[:n]]

    def map_merge(self, pairs, T, stamp_offset=0.0, seam_variance=None, hyps=None):
        """alego_map_merge: pairs (src, dst); T (n, 3, 4) or one for all; hyps: None or, per pair, the `hyp` list of map_align (or None).
        One dict per pair: status (2 merged, 0 empty source, -1 dropped frames, -3 does not fit), frames, points, loop_edges, cross_edges"""
        src, dst, n = _slot_list(pairs, pairs=True)
        T = np.asarray(T, np.float64)
        if T.ndim == 2:
            T = np.broadcast_to(T, (n,) + T.shape)
        T12 = np.ascontiguousarray(T.reshape(n, T.shape[-2] * T.shape[-1])[:, :12])
        sv = None if seam_variance is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seam_variance, np.float64), (6,)))
        opts = MapMergeOpts(float(stamp_offset), None if sv is None else sv.ctypes.data)
        hyp = None
        if hyps is not None:
            hyp = (MapAlignHyp * (max(n, 1) * ALIGN_MAX_QUERIES))()
            for i, hs in enumerate(hyps):
                for q, d in enumerate(hs or []):
                    _hyp_struct(hyp[i * ALIGN_MAX_QUERIES + q], d)
        out = (MapMergeResult * max(n, 1))()
        self._check(lib().alego_map_merge(self._h, src.ctypes.data, dst.ctypes.data, n, T12.ctypes.data, C.byref(opts), hyp, out), "alego_map_merge")
        return [dict(status=int(r.status), frames=int(r.frames), points=int(r.points), loop_edges=int(r.loop_edges), cross_edges=int(r.cross_edges)) for r in out[:n]]

    # ---- a slot's archive thinned in place on the device (needs map_enable) ----
    def map_thin(self, slots, min_dist):
        """alego_map_thin: one dict per slot: status (2 thinned, 1 nothing to drop, 0 no key frame, -1 dropped frames), frames_before, frames,
        points_before, points"""
        sl, n = _slot_list(slots)
        opts = MapThinOpts(float(min_dist))
        out = (MapThinResult * max(n, 1))()
        self._check(lib().alego_map_thin(self._h, sl.ctypes.data, n, C.byref(opts), out), "alego_map_thin")
        return [dict(status=int(r.status), frames_before=int(r.frames_before), frames=int(r.frames), points_before=int(r.points_before), points=int(r.points))
                for r in out[:n]]

    def debug_thin_select(self, keyposes6, protect, min_dist):
        """the selection kernel of alego_map_thin alone on the caller's arrays: the keep mask (n,) uint8"""
        kp, pr, keep = _thin_arrays(keyposes6, protect)
        rc = self._check(lib().alego_debug_thin_select(self._h, kp.ctypes.data, pr.ctypes.data, kp.shape[0], float(min_dist), keep.ctypes.data), "alego_debug_thin_select")
        assert rc == int(keep[:kp.shape[0]].sum())
        return keep[:kp.shape[0]]

    # ---- occupancy grid of the archive by ray casting (needs map_enable) ----
    def occ_enable(self, opts):
        """alego_occ_enable: opts from occ_opts(); once per handle"""
        self._check(lib().alego_occ_enable(self._h, C.byref(opts)), "alego_occ_enable")
        self._occ_opts = opts

    def occ_clear(self):
        self._check(lib().alego_occ_clear(self._h), "alego_occ_clear")

    def occ_integrate(self, kinds=7, first=0, n=-1, slot=0):
        """alego_occ_integrate: the call's counters (OCC_STATS,) int64"""
        stats = np.zeros(OCC_STATS, np.int64)
        self._check(lib().alego_occ_integrate(self._h, slot, first, n, kinds, stats.ctypes.data), "alego_occ_integrate")
        return stats

    def occ_get(self):
        """alego_occ_get: (hits, passes), each (n2, n1, n0) uint32"""
        shape = _occ_shape(self._occ_opts)
        hits, passes = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        self._check(lib().alego_occ_get(self._h, hits.ctypes.data, passes.ctypes.data), "alego_occ_get")
        return hits, passes

    def occ_classify(self, rule=None, collapse_z=False):
        """alego_occ_classify: int8 classes (n2, n1, n0), or (n1, n0) with collapse_z; rule = (min_hits, hit_weight, pass_weight) or None for the defaults"""
        out = np.zeros(_occ_shape(self._occ_opts, collapse_z), np.int8)
        self._check(lib().alego_occ_classify(self._h, _occ_rule(rule), int(bool(collapse_z)), out.ctypes.data), "alego_occ_classify")
        return out

    def occ_set(self, hits=None, passes=None):
        """alego_occ_set: copies counts (n2, n1, n0) uint32 to the grid; None keeps that array's counts"""
        shape = _occ_shape(self._occ_opts)
        h = None if hits is None else np.ascontiguousarray(hits, np.uint32)
        p = None if passes is None else np.ascontiguousarray(passes, np.uint32)
        assert all(a is None or a.shape == shape for a in (h, p))
        self._check(lib().alego_occ_set(self._h, None if h is None else h.ctypes.data, None if p is None else p.ctypes.data), "alego_occ_set")

    def occ_distance(self, rule=None, collapse_z=False, unknown_is_obstacle=False, max_cells=0, want_d2=True):
        """alego_occ_distance: (d2 uint32 (n2, n1, n0), or (n1, n0) with collapse_z, or None without want_d2; stats (EDT_STATS,) int64)"""
        o = OccDistOpts(int(bool(collapse_z)), int(bool(unknown_is_obstacle)), int(max_cells), 0)
        d2 = np.zeros(_occ_shape(self._occ_opts, collapse_z), np.uint32) if want_d2 else None
        stats = np.zeros(EDT_STATS, np.int64)
        self._check(lib().alego_occ_distance(self._h, _occ_rule(rule), C.byref(o), None if d2 is None else d2.ctypes.data, stats.ctypes.data), "alego_occ_distance")
        return d2, stats

    def occ_costmap(self, inflation, rule=None, collapse_z=False, unknown_is_obstacle=False):
        """alego_occ_costmap: uint8 costs (n2, n1, n0), or (n1, n0) with collapse_z; inflation from occ_inflation()"""
        out = np.zeros(_occ_shape(self._occ_opts, collapse_z), np.uint8)
        self._check(lib().alego_occ_costmap(self._h, _occ_rule(rule), int(bool(collapse_z)), int(bool(unknown_is_obstacle)), C.byref(inflation), out.ctypes.data),
                    "alego_occ_costmap")
        return out

    def occ_mark(self, kinds=7, rule=None, slot=0):
        """alego_occ_mark: (verdicts (n,) uint8 of the points of map_assemble(kinds & 7), stats (STATIC_VERDICTS,) int64); rule from static_rule() or None"""
        stats = np.zeros(STATIC_VERDICTS, np.int64)
        n = self._check(lib().alego_occ_mark(self._h, slot, kinds, _static_rule(rule), None, 0, None), "alego_occ_mark")
        verdict = np.zeros(max(n, 1), np.uint8)
        n = self._check(lib().alego_occ_mark(self._h, slot, kinds, _static_rule(rule), verdict.ctypes.data, n, stats.ctypes.data), "alego_occ_mark")
        return verdict[:n], stats

    def map_assemble_static(self, kinds, leaf=0.0, rule=None, slot=0, cap=None):
        """alego_map_assemble_static: (map_assemble's cloud without the points the grid saw through, stats (STATIC_VERDICTS,) int64)"""
        stats = np.zeros(STATIC_VERDICTS, np.int64)
        if cap is None:
            cap = self._check(lib().alego_map_assemble_static(self._h, slot, kinds, leaf, _static_rule(rule), None, 0, None), "alego_map_assemble_static")
        out = np.empty((max(cap, 1), 4), np.float32)
        n = self._check(lib().alego_map_assemble_static(self._h, slot, kinds, leaf, _static_rule(rule), out.ctypes.data, cap, stats.ctypes.data), "alego_map_assemble_static")
        return out[:n].copy(), stats

    def debug_occ_piece(self, piece):
        """development: steps of a ray one lane of occ_cast walks at a time (<= 0: one lane per ray)"""
        self._check(lib().alego_debug_occ_piece(self._h, int(piece)), "alego_debug_occ_piece")

    # ---- localisation against a frozen key-frame map ----
    def loc_enable(self, frames, radius=0.0):
        """frames = [(pose6, corner, surf, outlier), ...] (what map_get_keyframe returns, as tuples): every slot localises in them from now on"""
        keep, kfs = [], (KfIn * max(len(frames), 1))()
        for i, f in enumerate(frames):
            kfs[i].pose[:] = [float(v) for v in f[0]]
            arrs = [np.ascontiguousarray(c, np.float32).reshape(-1, 4) for c in f[1:4]]
            keep.append(arrs)
            kfs[i].corner, kfs[i].n_corner = arrs[0].ctypes.data, arrs[0].shape[0]
            kfs[i].surf, kfs[i].n_surf = arrs[1].ctypes.data, arrs[1].shape[0]
            kfs[i].outlier, kfs[i].n_outlier = arrs[2].ctypes.data, arrs[2].shape[0]
        self._check(lib().alego_loc_enable(self._h, kfs, len(frames), float(radius)), "alego_loc_enable")

    def loc_enable_from_map(self, map_handle, slot=0, radius=0.0, capacity=0):
        """the map store from the archive of `slot` of the mapping Handle `map_handle` as it is now, built on the device (capacity: frames allocated, 0 = as many as archived)"""
        self._check(lib().alego_loc_enable_from_map(self._h, map_handle._h if map_handle is not None else None, slot, float(radius), int(capacity)), "alego_loc_enable_from_map")

    def loc_update_from_map(self, map_handle, slot=0):
        """the whole store again from the archive as it is now; every slot's window is reset"""
        self._check(lib().alego_loc_update_from_map(self._h, map_handle._h if map_handle is not None else None, slot), "alego_loc_update_from_map")

    def loc_store_frame(self, f):
        """row f of the map store (debug read-outs): sorted runs, their counts and boxes, the raw clouds, the pose"""
        g = lambda name, cap: self.debug_get(f"{name}:{f}", cap_bytes=cap)
        big = 16 * self.N + 4096
        return dict(corner=g("ls_corner", big).reshape(-1, 4), surf=g("ls_surf", 2 * big).reshape(-1, 4), box_c=g("ls_box_c", 64), box_s=g("ls_box_s", 64),
                    raw_c=g("ls_raw_c", big).reshape(-1, 4), raw_s=g("ls_raw_s", big).reshape(-1, 4), raw_o=g("ls_raw_o", big).reshape(-1, 4),
                    pose=g("ls_pose", 64), counts=g("ls_counts", 64))

    def loc_status(self, slot=0):
        """dict(frames, window, rebuilds, optimized) of the slot's last mapping frame"""
        out = np.zeros(4, np.int32)
        self._check(lib().alego_loc_status(self._h, slot, out.ctypes.data), "alego_loc_status")
        return dict(frames=int(out[0]), window=int(out[1]), rebuilds=int(out[2]), optimized=int(out[3]))

    # ---- relocalisation in the frozen map (needs loc_enable) ----
    def reloc_enable(self, max_range=0.0, z_offset=float("nan")):
        self._check(lib().alego_reloc_enable(self._h, float(max_range), float(z_offset)), "alego_reloc_enable")

    def loc_relocalize(self, slots, n_cand=0, verify=-1, apply=False):
        """alego_loc_relocalize: one dict per listed slot (status, candidates, the verified candidate's ICP, t_map, rc, params6)"""
        sl, n = _slot_list(slots)
        out = (RelocResult * max(n, 1))()
        opts = RelocOpts(int(n_cand), int(verify), int(bool(apply)))
        self._check(lib().alego_loc_relocalize(self._h, sl.ctypes.data, n, C.byref(opts), out), "alego_loc_relocalize")
        return [_reloc_result(out[i]) for i in range(n)]

    def debug_reloc_search(self, map_desc, q_desc, n_cand):
        """the search kernels of alego_loc_relocalize alone: (ids, dists, shifts), each (n_q, n_cand) int32, -1 where the map has fewer frames"""
        m = np.ascontiguousarray(map_desc, np.uint8).reshape(-1, RELOC_SECTORS * RELOC_RINGS)
        q = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, RELOC_SECTORS * RELOC_RINGS)
        ids, dists, shifts = (np.zeros((q.shape[0], n_cand), np.int32) for _ in range(3))
        self._check(lib().alego_debug_reloc_search(self._h, m.ctypes.data, m.shape[0], q.ctypes.data, q.shape[0], int(n_cand), ids.ctypes.data,
                                                   dists.ctypes.data, shifts.ctypes.data), "alego_debug_reloc_search")
        return ids, dists, shifts

    # ---- the key-pose graph (needs map_enable) ----
    def graph_enable(self, max_loops, odom_variance=None):
        v = None if odom_variance is None else np.ascontiguousarray(odom_variance, np.float64).reshape(6)
        self._check(lib().alego_graph_enable(self._h, int(max_loops), None if v is None else v.ctypes.data), "alego_graph_enable")

    def graph_get_edges(self, kind=0, first=0, n=None, slot=0):
        """dict(frm, to, between (n, 3, 4), variance (n, 6)); kind 0: the chain (edge 0 = the prior), 1: the loop edges; n = None: all"""
        if n is None:
            n = self.graph_status(slot)[0 if kind == 0 else 1] - first
        e = (GraphEdge * max(n, 1))()
        self._check(lib().alego_graph_get_edges(self._h, slot, kind, first, n, e), "alego_graph_get_edges")
        return _graph_edges_out(e, n)

    def graph_status(self, slot=0):
        """(chain edges, loop edges, loop_closed_, poses of the last estimate)"""
        out = np.zeros(4, np.int32)
        self._check(lib().alego_graph_status(self._h, slot, out.ctypes.data), "alego_graph_status")
        return tuple(int(v) for v in out)

    def graph_set_edges(self, first, frm, to, between, variance, slot=0):
        e = graph_edges(frm, to, between, variance)
        self._check(lib().alego_graph_set_edges(self._h, slot, first, len(np.asarray(frm).reshape(-1)), e), "alego_graph_set_edges")

    def graph_add_loops(self, slots, results):
        """results: the dicts loop_search returned for `slots`; entries with status == 2 are appended"""
        sl, n = _slot_list(slots)
        r = (LoopResult * max(n, 1))()
        for i, d in enumerate(results):
            r[i].status, r[i].latest_id, r[i].closest_id = d["status"], d["latest_id"], d["closest_id"]
            r[i].fitness, r[i].noise_variance = d["fitness"], d["noise_variance"]
            r[i].correction[:] = np.asarray(d["T"], np.float32).reshape(16).tolist()
            r[i].between[:] = np.asarray(d["between"], np.float64).reshape(12).tolist()
        self._check(lib().alego_graph_add_loops(self._h, sl.ctypes.data, n, r), "alego_graph_add_loops")

    def graph_add_edge(self, frm, to, between, variance, correction=None, slot=0):
        e = graph_edges([frm], [to], [between], [variance])
        c = None if correction is None else np.ascontiguousarray(correction, np.float32).reshape(16)
        self._check(lib().alego_graph_add_edge(self._h, slot, e, None if c is None else c.ctypes.data), "alego_graph_add_edge")

    def graph_optimize(self, slots, max_iters=0, step_tol=0.0, apply=False):
        """alego_graph_optimize: one dict per listed slot (status, iterations, n_poses, n_loops, applied, cost0, cost, last_step);
        max_iters / step_tol 0 = the library's defaults"""
        sl, n = _slot_list(slots)
        o = GraphOpts(int(max_iters), float(step_tol), int(bool(apply)))
        out = (GraphResult * max(n, 1))()
        self._check(lib().alego_graph_optimize(self._h, sl.ctypes.data, n, C.byref(o), out), "alego_graph_optimize")
        return [dict(status=int(r.status), iterations=int(r.iterations), n_poses=int(r.n_poses), n_loops=int(r.n_loops), applied=int(r.applied),
                     cost0=float(r.cost0), cost=float(r.cost), last_step=float(r.last_step)) for r in out[:n]]

    def graph_get_estimate(self, first=0, n=None, slot=0):
        """(n, 3, 4) f64 poses of the slot's last optimise"""
        if n is None:
            n = self.map_status(slot)[0] - first
        out = np.zeros((max(n, 1), 12), np.float64)
        self._check(lib().alego_graph_get_estimate(self._h, slot, first, n, out.ctypes.data), "alego_graph_get_estimate")
        return out[:n].reshape(n, 3, 4)

    def graph_marginals(self, slots, cap=None):
        """alego_graph_marginals: (one dict (status, n_poses, n_loops) per listed slot, cov (n, cap, 6, 6)); cap = None: the longest archive listed"""
        sl, n = _slot_list(slots)
        if cap is None:
            cap = max([self.map_status(int(s))[0] for s in sl] + [1])
        cov = np.zeros((max(n, 1), max(int(cap), 1), 36), np.float64)
        out = (GraphCovResult * max(n, 1))()
        self._check(lib().alego_graph_marginals(self._h, sl.ctypes.data, n, int(cap), cov.ctypes.data, out), "alego_graph_marginals")
        return ([dict(status=int(r.status), n_poses=int(r.n_poses), n_loops=int(r.n_loops)) for r in out[:n]],
                cov[:n].reshape(n, max(int(cap), 1), 6, 6))

    def graph_check_edges(self, slots, frm, to, between, variance):
        """alego_graph_check_edges: candidate i for slots[i]; one dict (status, d2, error (6,), cov (6, 6)) per candidate"""
        sl, n = _slot_list(slots)
        out = (GraphCheck * max(n, 1))()
        self._check(lib().alego_graph_check_edges(self._h, sl.ctypes.data, n, graph_edges(frm, to, between, variance), out), "alego_graph_check_edges")
        return _graph_checks_out(out, n)

    def graph_check_loops(self, slots, results):
        """alego_graph_check_loops: the edge graph_add_loops would append for every dict of loop_search (status == 2; others give status 0)"""
        sl, n = _slot_list(slots)
        r = (LoopResult * max(n, 1))()
        for i, d in enumerate(results):
            r[i].status, r[i].latest_id, r[i].closest_id = d["status"], d["latest_id"], d["closest_id"]
            r[i].fitness, r[i].noise_variance = d["fitness"], d["noise_variance"]
            r[i].between[:] = np.asarray(d["between"], np.float64).reshape(12).tolist()
        out = (GraphCheck * max(n, 1))()
        self._check(lib().alego_graph_check_loops(self._h, sl.ctypes.data, n, r, out), "alego_graph_check_loops")
        return _graph_checks_out(out, n)

    def debug_nn1(self, tgt, queries):
        """the grid 1-NN of alego_loop_search alone: (index, f32 squared distance) per query"""
        t = np.ascontiguousarray(tgt, np.float32).reshape(-1, 4)
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)
        idx = np.zeros(max(q.shape[0], 1), np.int32)
        d2 = np.zeros(max(q.shape[0], 1), np.float32)
        self._check(lib().alego_debug_nn1(self._h, t.ctypes.data, t.shape[0], q.ctypes.data, q.shape[0], idx.ctypes.data, d2.ctypes.data), "alego_debug_nn1")
        return idx[:q.shape[0]].copy(), d2[:q.shape[0]].copy()

    # ---- one registration sharded over the ranks of an RCCL communicator (BASELINE config 5) ----
    # ---- covariance and degeneracy of the scan-to-map registration ----
    def regcov_enable(self, opts=None):
        """alego_regcov_enable: opts = regcov_opts(...) or None for the defaults; before the first scan reaches LaserMapping"""
        self._check(lib().alego_regcov_enable(self._h, None if opts is None else C.byref(opts)), "alego_regcov_enable")

    def _records_get(self, name, Rec, shapes, slots):
        """a slot-list *_get: one record dict per listed slot"""
        sl, n = _slot_list(slots)
        out = (Rec * max(n, 1))()
        self._check(getattr(lib(), name)(self._h, sl.ctypes.data, n, out), name)
        return [_record_out(r, shapes) for r in out[:n]]

    def regcov_get(self, slots=(0,)):
        """alego_regcov_get: one dict per listed slot (status, n_edge, n_plane, n_degenerate, frame, cost, sigma2, info, eigval, eigvec, cov, variance)"""
        return self._records_get("alego_regcov_get", RegCov, _REGCOV_SHAPES, slots)

    def remap_enable(self, opts=None):
        """alego_remap_enable: opts = remap_opts(eig_min) or None for the default; before the first scan reaches LaserMapping"""
        self._check(lib().alego_remap_enable(self._h, None if opts is None else C.byref(opts)), "alego_remap_enable")

    def remap_get(self, slots=(0,)):
        """alego_remap_get: one dict per listed slot (status, n_held, frame, start, eigval, eigvec, proj)"""
        return self._records_get("alego_remap_get", Remap, _REMAP_SHAPES, slots)

    def debug_remap_solve(self, start6, edge_rows9, plane_rows7, remap=1):
        """alego_debug_remap_solve: the solver kernel alone (remap = 0: lm_solve, 1: lm_solve_remap) on rows (a, b, p) (n, 9) and (n, d, p) (m, 7) from
        start6 -> dict(params_it (2, 6), costs (4,), iterations, successful, termination (2,) each, rec)"""
        p = np.ascontiguousarray(start6, np.float64).reshape(6)
        e, s = np.ascontiguousarray(edge_rows9, np.float64).reshape(-1, 9), np.ascontiguousarray(plane_rows7, np.float64).reshape(-1, 7)
        pit, costs, summ, rec = np.zeros((2, 6)), np.zeros(4), np.zeros(2, np.int32), Remap()
        self._check(lib().alego_debug_remap_solve(self._h, p.ctypes.data, e.ctypes.data if len(e) else None, len(e), s.ctypes.data if len(s) else None, len(s), int(remap),
                                                  pit.ctypes.data, costs.ctypes.data, summ.ctypes.data, C.byref(rec)), "alego_debug_remap_solve")
        return dict(params_it=pit, costs=costs, iterations=summ & 0xFF, successful=(summ >> 8) & 0xFF, termination=summ >> 16, rec=_record_out(rec, _REMAP_SHAPES))

    def debug_regcov(self, params6, edge_rows9, plane_rows7):
        """alego_debug_regcov: lm_regcov alone on rows (a, b, p) (n, 9) and (n, d, p) (m, 7) at params6 (p is rounded to f32)"""
        p = np.ascontiguousarray(params6, np.float64).reshape(6)
        e, s = np.ascontiguousarray(edge_rows9, np.float64).reshape(-1, 9), np.ascontiguousarray(plane_rows7, np.float64).reshape(-1, 7)
        out = RegCov()
        self._check(lib().alego_debug_regcov(self._h, p.ctypes.data, e.ctypes.data if len(e) else None, len(e), s.ctypes.data if len(s) else None, len(s), C.byref(out)),
                    "alego_debug_regcov")
        return _record_out(out, _REGCOV_SHAPES)

    def dist_init(self, rank, world, unique_id: bytes):
        self._check(lib().alego_dist_init(self._h, rank, world, C.create_string_buffer(unique_id, DIST_ID_BYTES)), "alego_dist_init")

    def dist_allreduce_probe(self, iters=200):
        """microseconds per ncclAllReduce of one solver evaluation's 32 doubles (a collective: every rank calls it)"""
        us = C.c_double()
        self._check(lib().alego_dist_allreduce_probe(self._h, iters, C.byref(us)), "alego_dist_allreduce_probe")
        return float(us.value)

    def dist_shutdown(self):
        self._check(lib().alego_dist_shutdown(self._h), "alego_dist_shutdown")

    # ---- key-frame pass-through (host pose graph) ----
    def lm_keyframe_count(self, slot=0):
        return self._check(lib().alego_lm_keyframe_count(self._h, slot), "alego_lm_keyframe_count")

    def lm_get_keyframe(self, kf_id=-1, slot=0):
        """dict(id, pose[6], corner, surf, outlier): a resident key frame as saveKeyFramesAndFactor stored it"""
        N = self.N
        bufs = [np.empty((N, 4), np.float32) for _ in range(3)]
        k = KeyFrame()
        k.corner, k.corner_cap = bufs[0].ctypes.data, N
        k.surf, k.surf_cap = bufs[1].ctypes.data, N
        k.outlier, k.outlier_cap = bufs[2].ctypes.data, N
        self._check(lib().alego_lm_get_keyframe(self._h, slot, kf_id, C.byref(k)), "alego_lm_get_keyframe")
        return dict(id=int(k.id), pose=np.array(k.pose[:], np.float32), corner=bufs[0][:k.n_corner].copy(), surf=bufs[1][:k.n_surf].copy(),
                    outlier=bufs[2][:k.n_outlier].copy())

    def lm_set_keypose(self, kf_id, pose6, slot=0):
        a = np.ascontiguousarray(pose6, np.float32)
        self._check(lib().alego_lm_set_keypose(self._h, slot, kf_id, a.ctypes.data), "alego_lm_set_keypose")

    def lm_reset_window(self, slot=0):
        self._check(lib().alego_lm_reset_window(self._h, slot), "alego_lm_reset_window")

    def lm_apply_correction(self, rc12, slot=0):
        a = np.ascontiguousarray(rc12, np.float64).reshape(12)
        self._check(lib().alego_lm_apply_correction(self._h, slot, a.ctypes.data), "alego_lm_apply_correction")

    def lm_add_keyframe(self, pose6, corner, surf, outlier, slot=0):
        a = np.ascontiguousarray(pose6, np.float32)
        c, s, o = (np.ascontiguousarray(v, np.float32).reshape(-1, 4) for v in (corner, surf, outlier))
        self._check(lib().alego_lm_add_keyframe(self._h, slot, a.ctypes.data, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0],
                                                o.ctypes.data, o.shape[0]), "alego_lm_add_keyframe")

    def atan2f(self, y, x):
        y = np.ascontiguousarray(y, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(y)
        self._check(lib().alego_debug_atan2f(self._h, y.ctypes.data, x.ctypes.data, out.ctypes.data, y.size), "alego_debug_atan2f")
        return out
