"""Localisation mode (alego_loc_select / alego_loc_enable / alego_loc_status, kernels_loc.hip): many streams
registered against one frozen key-frame map.

The selection rule is restated in numpy f32 with the same operation order.  A localisation frame is emulated with the UNCHANGED oracle:
a fresh Oracle whose min_keyframe_dist is 1e18 (it never saves a key frame) gets the window's frames with lm_add_keyframe in id order (K
frames fit its window), the slot's map -> odom of before the frame with lm_apply_correction on its identity, the slot's params_ of before
the frame with set_lm_params (params_ persists between frames on the device as it does in the reference; a fresh oracle starts at zero),
and the frame's clouds and odometry with lm_process.  _lm_compare reads the device's key-frame count (lm_info[0]) against the oracle's:
localisation keeps it at 0 on purpose while the emulation holds the window's frames, so the comparison sees the device through a view
that reports the window size there; the 0 itself is asserted separately.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal, quat_angle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAP = 560
LI_NKF, LI_RUN, LI_KF_ADDED, LI_OPTIMIZED, LI_NREBUILD, LI_REC_CNT = 0, 2, 10, 11, 24, 26   # (lm_ctx.h)
LD_M2O, LD_LOC_P = 6, 44
NEW_SYMBOLS = ["alego_loc_select", "alego_loc_enable", "alego_loc_status"]
# (K, radius) of the three lap runs: K binds / the radius binds / everything is selected
CONFIGS = [(10, 6.0), (10, 4.0), (50, 50.0)]
EMPTY = np.zeros((0, 4), F32)


def _O():
    from oracle import oracle_py
    return oracle_py


# ---- the rule in numpy --------------------------------------------------------------------------------------------------------
def select_np(keyposes6, xyz, radius, k):
    kp = np.ascontiguousarray(keyposes6, F32).reshape(-1, 6)
    p = np.ascontiguousarray(xyz, F32).reshape(3)
    if not np.isfinite(p).all() or kp.shape[0] == 0:
        return np.zeros(0, np.int32)
    r = radius if radius > 0 else 50.0
    r2 = F32(r * r)
    dx, dy, dz = kp[:, 0] - p[0], kp[:, 1] - p[1], kp[:, 2] - p[2]
    d2 = ((dx * dx) + dy * dy) + dz * dz
    assert d2.dtype == F32
    cand = np.nonzero(d2 < r2)[0]
    key = (d2[cand].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)
    keep = cand[np.argsort(key, kind="stable")[:k]]
    return np.sort(keep).astype(np.int32)


def n_candidates(keyposes6, xyz, radius):
    return len(select_np(keyposes6, xyz, radius, 1 << 30))


def _poses(xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    return np.c_[xyz, np.zeros((len(xyz), 3), F32)].astype(F32)


def rule_cases():
    """(name, keyposes6, position, radius, K)"""
    rng = np.random.default_rng(7)
    out = []
    rnd = _poses(rng.uniform(-20, 20, (300, 3)))
    for i in range(6):
        out.append((f"random {i}", rnd, rng.uniform(-15, 15, 3).astype(F32), float(rng.uniform(3, 25)), int(rng.integers(1, 60))))
    dup = _poses([[1, 0, 0]] * 6 + [[0, 1, 0]] * 6 + [[0, 0, 0.5]])
    out.append(("duplicates: the lowest ids win", dup, np.zeros(3, F32), 5.0, 4))
    out.append(("duplicates across the cut", dup, np.zeros(3, F32), 5.0, 8))
    # d2 exactly r2: 3-4-0 at radius 5 (all exact in f32) is excluded, the frame just inside is kept
    edge = _poses([[3, 4, 0], [3, 3.9990234375, 0], [0, 0, 5], [0, 0, 0]])
    out.append(("d2 == r2 is excluded", edge, np.zeros(3, F32), 5.0, 10))
    line = _poses([[i, 0, 0] for i in range(12)])
    out.append(("more than K", line, np.zeros(3, F32), 7.5, 5))
    out.append(("exactly K", line, np.zeros(3, F32), 4.5, 5))
    out.append(("fewer than K", line, np.zeros(3, F32), 2.5, 5))
    out.append(("no candidates", line, np.array([0, 100, 0], F32), 2.5, 5))
    out.append(("n = 0", _poses(np.zeros((0, 3))), np.zeros(3, F32), 5.0, 5))
    out.append(("K = 1", line, np.array([6.2, 0, 0], F32), 5.0, 1))
    out.append(("K >= n", line, np.array([6.2, 0, 0], F32), 50.0, 12))
    out.append(("K > n", line, np.array([6.2, 0, 0], F32), 50.0, 40))
    out.append(("radius <= 0 is 50", line, np.array([45.0, 0, 0], F32), 0.0, 40))
    out.append(("NaN position", line, np.array([np.nan, 0, 0], F32), 5.0, 5))
    out.append(("infinite position", line, np.array([0, np.inf, 0], F32), 5.0, 5))
    return out


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_localisation_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s


def test_loc_select_rule_vs_numpy():
    seen = set()
    for name, kp, p, radius, k in rule_cases():
        got = binding.loc_select(kp, p, radius, k)
        want = select_np(kp, p, radius, k)
        assert np.array_equal(got, want), (name, got, want)
        nc = n_candidates(kp, p, radius)
        seen.add("more" if nc > k else "exact" if nc == k and nc > 0 else "fewer" if nc > 0 else "none")
        if name.startswith("duplicates: the lowest"):
            assert got.tolist() == [0, 1, 2, 12], got   # z = 0.5 is nearest, then three of the six at distance 1 with the lowest ids
        if name.startswith("d2 == r2"):
            assert got.tolist() == [1, 3], got
        if name.startswith(("NaN", "infinite", "no candidates", "n = 0")):
            assert len(got) == 0
        if name == "K >= n":
            assert got.tolist() == list(range(12))
    assert seen == {"more", "exact", "fewer", "none"}, seen


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _quat_R(q):
    w, x, y, z = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _rc(t, q=(1.0, 0.0, 0.0, 0.0)):
    return np.c_[_quat_R(q), np.asarray(t, np.float64).reshape(3)].reshape(12)


def _euler_zyx(q):
    R = _quat_R(q)
    return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[2, 1], R[2, 2])), np.arctan2(R[1, 0], R[0, 0])])


def _params(k=None, **kw):
    p = synth.default_params(16, 1800)
    if k is not None:
        p.recent_keyframe_num = k
    for name, v in kw.items():
        setattr(p, name, v)
    return p


_SCANS = {}


def _scan(k):
    if k not in _SCANS:
        _SCANS[k] = synth.scan(_params(), k)
    return _SCANS[k]


class _WindowAsKeyFrames:
    """the device as _lm_compare reads it, with the window size where SLAM mode has its key-frame count (module docstring)"""

    def __init__(self, h, nwin):
        self._h, self._n, self.params = h, nwin, h.params

    def debug_get(self, name, *a, **kw):
        out = self._h.debug_get(name, *a, **kw)
        if name == "lm_info":
            assert out[LI_NKF] == 0, "a localising slot saved a key frame"
            out = out.copy()
            out[LI_NKF] = self._n
        return out


def emulate(pl, frames, window, m2o7, params6, corner, surf, outlier, odom7):
    """one localisation frame on a fresh oracle; the caller closes it"""
    O = _O()
    pe = type(pl).from_buffer_copy(pl)
    pe.min_keyframe_dist = 1e18
    e = O.Oracle(pe)
    for i in window:
        e.lm_add_keyframe(frames[i]["pose"], frames[i]["corner"], frames[i]["surf"], frames[i]["outlier"])
    e.lm_apply_correction(_rc(m2o7[:3], m2o7[3:]))
    e.set_lm_params(params6)
    e.lm_process(corner, surf, outlier, odom7)
    return e


# (a slot is placed through alego_lm_apply_correction: the two non-finite positions stay with the CPU test)
PLACED = [i for i, c in enumerate(rule_cases()) if np.isfinite(c[2]).all()]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLACED)
def test_selection_kernel_equals_the_host_rule(case):
    name, kp, pos, radius, k = rule_cases()[case]
    p = _params(k, lm_every=1)
    h = binding.Handle(p)
    rng = np.random.default_rng(case)
    tiny = lambda n: np.c_[rng.uniform(-1, 1, (n, 3)), np.zeros(n)].astype(F32)
    h.loc_enable([(q, tiny(i % 3), tiny((i + 1) % 3), EMPTY) for i, q in enumerate(kp)], radius)
    h.lm_apply_correction(_rc(pos.astype(np.float64)))
    flags, mp = h.lm_process(EMPTY, EMPTY, EMPTY, dict(t=[0, 0, 0], q=[1, 0, 0, 0]))
    assert not flags & binding.FLAG_LM_KEYFRAME
    st = h.debug_get("lm_state")
    got_p = st[LD_LOC_P:LD_LOC_P + 3]
    assert_bit_equal(got_p.astype(F32), pos.astype(F32), f"{name}: p")
    assert np.array_equal(got_p, got_p.astype(F32).astype(np.float64))
    win = h.debug_get("lm_window")
    assert np.array_equal(win, binding.loc_select(kp, got_p.astype(F32), radius, k)), (name, win)
    assert np.array_equal(win, select_np(kp, pos, radius, k)), (name, win)
    s = h.loc_status()
    assert (s["frames"], s["window"], s["optimized"]) == (len(kp), len(win), 0), (name, s)
    assert s["rebuilds"] == (1 if len(win) else 0), (name, s)
    assert h.lm_keyframe_count() == 0
    h.close()


@pytest.fixture(scope="module")
def lap_map():
    """the lap mapped once on a SLAM handle with the archive on: its key frames and its map pose of every scan"""
    p = _params()
    h = binding.Handle(p)
    h.map_enable(256, 1 << 20)
    track = np.zeros((LAP, 7))
    for k in range(LAP):
        flags, odom, mp = h.scan_process(_scan(k), stages=7)
        track[k] = np.r_[mp["t"], mp["q"]]
    nf, dropped = h.map_status()[:2]
    assert dropped == 0 and nf >= 40, (nf, dropped)
    frames = [h.map_get_keyframe(i) for i in range(nf)]
    h.close()
    kp = np.array([f["pose"] for f in frames], F32).reshape(-1, 6)
    return dict(frames=frames, kp=kp, track=track)


_RUNS = {}


def _device_run(lap_map, cfg, compare):
    """the lap on a one-slot localising handle.  compare: every mapping frame against the teacher-forced emulation.  Returns the record of
    the run: per scan the clouds LaserMapping got, the odometry, the map pose and whether the body ran."""
    from test_gpu_parity import POSE_TOL, _lm_compare
    K, radius = cfg
    frames, kp = lap_map["frames"], lap_map["kp"]
    pl = _params(K)
    h = binding.Handle(pl)
    h.loc_enable([(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames], radius)
    rec, windows, ncand = [], [], []
    for k in range(LAP):
        st0 = h.debug_get("lm_state")
        flags, odom, mp, seg, feat = h.scan_process(_scan(k), stages=7, want_outputs=True)
        assert flags >= 0 and not flags & binding.FLAG_LM_KEYFRAME, (cfg, k, flags)
        gi = h.debug_get("lm_info")
        ran = bool(gi[LI_RUN])
        rec.append(dict(corner=feat["less_sharp"], surf=feat["less_flat"], outlier=seg["outlier"], odom=np.r_[odom["t"], odom["q"]],
                        mp=np.r_[mp["t"], mp["q"]], ran=ran, valid=k > 0))
        if not ran:
            continue
        st1 = h.debug_get("lm_state")
        pf = st1[LD_LOC_P:LD_LOC_P + 3].astype(F32)
        win = h.debug_get("lm_window")
        tag = f"K {K} radius {radius} scan {k}"
        assert np.array_equal(win, binding.loc_select(kp, pf, radius, K)), (tag, win)
        assert np.array_equal(win, select_np(kp, pf, radius, K)), (tag, win)
        assert_bit_equal(pf, mp["t"].astype(F32), f"{tag}: p is the f32 of t_map2laser_ after transformAssociateToMap")
        windows.append(win)
        ncand.append(n_candidates(kp, pf, radius))
        if compare:
            e = emulate(pl, frames, win, st0[LD_M2O:LD_M2O + 7], st0[0:6], rec[-1]["corner"], rec[-1]["surf"], rec[-1]["outlier"], rec[-1]["odom"])
            _lm_compare(_WindowAsKeyFrames(h, len(win)), e, k, tag)
            want = e.get("map_pose")
            assert np.abs(mp["t"] - want[:3]).max() < POSE_TOL and quat_angle(mp["q"], want[3:]) < POSE_TOL, (tag, mp["t"], want)
            m2o = e.get("lm_map2odom")
            assert np.abs(st1[LD_M2O:LD_M2O + 3] - m2o[:3]).max() < POSE_TOL and quat_angle(st1[LD_M2O + 3:LD_M2O + 7], m2o[3:]) < POSE_TOL, (tag, st1[6:13], m2o)
            assert bool(gi[LI_OPTIMIZED]) == bool(e.get("lm_info")[1]) and not e.get("lm_info")[2], tag
            e.close()
        assert h.loc_status()["window"] == len(win) and h.loc_status()["optimized"] == int(gi[LI_OPTIMIZED])
    assert h.lm_keyframe_count() == 0
    changes = sum(1 for a, b in zip(windows, windows[1:]) if not np.array_equal(a, b))
    nreb = h.loc_status()["rebuilds"]
    h.close()
    out = dict(rec=rec, windows=windows, ncand=ncand, changes=changes, rebuilds=nreb, pl=pl)
    _RUNS[cfg] = out
    return out


def _assert_premises(cfg, run, n_frames):
    K, radius = cfg
    ncand, windows = np.array(run["ncand"]), run["windows"]
    print(f"K {K} radius {radius}: {len(windows)} mapping frames, candidates {ncand.min()}..{ncand.max()}, window changes {run['changes']}, rebuilds {run['rebuilds']}")
    assert run["rebuilds"] == run["changes"] + 1, "an unchanged window must not cost a rebuild (+ 1: the first window)"
    if cfg == CONFIGS[0]:
        assert (ncand > K).any() and run["changes"] > 0, "K binds on some frames"
        assert all(len(w) == min(K, c) for w, c in zip(windows, ncand))
    elif cfg == CONFIGS[1]:
        assert (ncand <= K).all() and (ncand < n_frames).all() and (ncand > 0).all() and run["changes"] > 0, "the radius binds on every frame"
    else:
        assert all(len(w) == n_frames for w in windows) and run["changes"] == 0, "every frame is selected on every mapping frame"


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_lap_teacher_forced_against_the_oracle(lap_map, cfg):
    run = _device_run(lap_map, cfg, compare=True)
    _assert_premises(cfg, run, len(lap_map["frames"]))
    assert sum(r["ran"] for r in run["rec"]) == (LAP - 1 + 1) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
def test_lap_free_run_against_the_chained_emulation(lap_map, cfg):
    """device: the free run of _device_run.  CPU: the emulation chained on itself — every frame's map -> odom and params_ are the previous
    emulated frame's, its window is the host rule at its own pose.  The chained emulation alone stays 0.033 - 0.040 m from the mapping run's
    poses; 0.1 m is the bound a stream that lost the map breaks."""
    from test_gpu_parity import POSE_TOL
    K, radius = cfg
    run = _RUNS.get(cfg) or _device_run(lap_map, cfg, compare=False)
    frames, kp, track = lap_map["frames"], lap_map["kp"], lap_map["track"]
    m2o, params = np.r_[0.0, 0, 0, 1, 0, 0, 0], np.zeros(6)
    worst, worst_dev, worst_emu = 0.0, 0.0, 0.0
    for k, r in enumerate(run["rec"]):
        if not r["valid"]:
            continue
        want_t = _quat_R(m2o[3:]) @ r["odom"][:3] + m2o[:3]
        if r["ran"]:
            win = binding.loc_select(kp, want_t.astype(F32), radius, K)
            e = emulate(run["pl"], frames, win, m2o, params, r["corner"], r["surf"], r["outlier"], r["odom"])
            want_t = e.get("map_pose")[:3]
            m2o, params = e.get("lm_map2odom"), e.get("lm_params")
            assert not e.get("lm_info")[2]
            e.close()
        worst = max(worst, np.abs(r["mp"][:3] - want_t).max())
        worst_dev = max(worst_dev, np.abs(r["mp"][:3] - track[k, :3]).max())
        worst_emu = max(worst_emu, np.abs(want_t - track[k, :3]).max())
    print(f"K {K} radius {radius}: device vs chained emulation {worst:.3e} m; from the mapping run: device {worst_dev:.4f} m, emulation {worst_emu:.4f} m")
    assert worst < POSE_TOL, worst
    assert worst_dev < 0.1 and worst_emu < 0.1, (worst_dev, worst_emu)


@pytest.mark.gpu
def test_off_the_map_is_dead_reckoning(lap_map):
    from test_gpu_parity import POSE_TOL, _lm_compare
    frames, kp = lap_map["frames"], lap_map["kp"]
    pl = _params(10)
    h = binding.Handle(pl)
    h.loc_enable([(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames], 6.0)
    c = np.array([kp[:, 0].max() + 100.0, kp[:, 1].max() + 100.0, 3.0])
    h.lm_apply_correction(_rc(c))
    m2o0 = h.debug_get("lm_state")[LD_M2O:LD_M2O + 7].copy()
    for k in range(20):
        flags, odom, mp = h.scan_process(_scan(k), stages=7)
        assert not flags & binding.FLAG_LM_KEYFRAME
        st, gi, s = h.debug_get("lm_state"), h.debug_get("lm_info"), h.loc_status()
        assert len(h.debug_get("lm_window")) == 0 and (s["window"], s["optimized"], s["rebuilds"]) == (0, 0, 0), (k, s)
        assert not gi[LI_OPTIMIZED] and gi[LI_NKF] == 0
        assert_bit_equal(st[LD_M2O:LD_M2O + 7], m2o0, f"scan {k}: map -> odom")
        if k > 0:
            np.testing.assert_allclose(mp["t"], np.asarray(odom["t"]) + c, rtol=0, atol=1e-12, err_msg=f"scan {k}")
            np.testing.assert_allclose(mp["q"], odom["q"], rtol=0, atol=1e-12, err_msg=f"scan {k}")   # (map -> odom has no rotation here)
    assert len(h.lm_local_map()[0]) == 0
    h.close()
    # a map that is there but too thin: no corner points, so every window stays below lm_min_map_corner and the oracle skips as well
    assert pl.lm_min_map_corner > 0
    thin = [dict(pose=f["pose"], corner=EMPTY, surf=f["surf"], outlier=f["outlier"]) for f in frames]
    h = binding.Handle(pl)
    h.loc_enable([(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in thin], 6.0)
    ran = 0
    for k in range(12):
        st0 = h.debug_get("lm_state")
        flags, odom, mp, seg, feat = h.scan_process(_scan(k), stages=7, want_outputs=True)
        gi = h.debug_get("lm_info")
        if not gi[LI_RUN]:
            continue
        ran += 1
        win = h.debug_get("lm_window")
        assert len(win) > 0 and not gi[LI_OPTIMIZED] and flags & binding.FLAG_LM_FEW_FEATURES, (k, win, flags)
        e = emulate(pl, thin, win, st0[LD_M2O:LD_M2O + 7], st0[0:6], feat["less_sharp"], feat["less_flat"], seg["outlier"], np.r_[odom["t"], odom["q"]])
        assert not e.get("lm_info")[1]
        _lm_compare(_WindowAsKeyFrames(h, len(win)), e, k, f"thin map scan {k}")
        want, m2o = e.get("map_pose"), e.get("lm_map2odom")
        st1 = h.debug_get("lm_state")
        assert np.abs(mp["t"] - want[:3]).max() < POSE_TOL and quat_angle(mp["q"], want[3:]) < POSE_TOL
        assert np.abs(st1[LD_M2O:LD_M2O + 3] - m2o[:3]).max() < POSE_TOL and quat_angle(st1[LD_M2O + 3:LD_M2O + 7], m2o[3:]) < POSE_TOL
        e.close()
    assert ran >= 5
    h.close()


@pytest.mark.gpu
def test_many_slots_one_map_match_single_slot_replicas(lap_map):
    """128 slots in two stream groups replay the lap from the bag store, from different start scans, against ONE map store; the first two and
    the last slot of every group equal one-slot localising replicas bit for bit (trajectory log, last local maps, lm_info, lm_state)."""
    frames, track = lap_map["frames"], lap_map["track"]
    pl = _params(10)
    n_slots, steps, radius = 128, 120, 6.0   # 60 mapping frames per slot: about a dozen window changes each
    start = lambda s: (s * 37) % LAP
    fr = [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames]

    def replay(starts, sync):
        h = binding.Handle(pl, n_slots=len(starts))
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, _scan(k))
        h.trajectory_enable(steps)
        h.loc_enable(fr, radius)
        for s, st in enumerate(starts):
            h.replay_assign(s, 0, st)
            h.lm_apply_correction(_rc(track[st, :3], track[st, 3:]), slot=s)   # the mapping run's map pose of the slot's first scan
            h.set_lm_params(np.r_[track[st, :3], _euler_zyx(track[st, 3:])], slot=s)
        h.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=sync)
        h.synchronize()
        return h

    h = replay([start(s) for s in range(n_slots)], False)
    groups, per = h.stream_groups()
    assert groups >= 2
    for s in range(n_slots):
        h.batch_get_pose(s)   # (raises on a capacity error of the slot)
        assert h.lm_keyframe_count(s) == 0
    optimised = 0
    for g in range(groups):
        for s in (g * per, g * per + 1, min(n_slots, (g + 1) * per) - 1):
            r = replay([start(s)], True)
            r.batch_get_pose(0)
            assert_bit_equal(h.trajectory(s), r.trajectory(0), f"slot {s} trajectory log")
            for name in ("lm_corner_map_ds", "lm_surf_map_ds", "lm_info", "lm_state", "lm_window"):
                assert_bit_equal(h.debug_get(name, slot=s), r.debug_get(name), f"slot {s} {name}")
            assert h.loc_status(s) == r.loc_status(0)
            optimised += h.loc_status(s)["optimized"]
            assert h.loc_status(s)["rebuilds"] >= 5, (s, h.loc_status(s))
            r.close()
    assert optimised > 0
    h.close()


@pytest.mark.gpu
def test_mode_boundaries(lap_map):
    frames = lap_map["frames"]
    fr = [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames[:4]]
    p = _params(10)

    def refused(fn, code=binding.ERR_ARG, text=None):
        with pytest.raises(binding.AlegoError) as ei:
            fn()
        assert f"({code})" in str(ei.value), ei.value
        if text:
            assert text in str(ei.value), ei.value

    h = binding.Handle(p)
    refused(lambda: h.loc_status())                       # not localising
    h.loc_enable(fr, 0.0)
    refused(lambda: h.loc_enable(fr, 0.0))                # a second call
    refused(lambda: h.map_enable(16, 1 << 16))
    refused(lambda: h.graph_enable(4))
    for fn in (lambda: h.map_status(), lambda: h.map_get_keyframe(0), lambda: h.map_assemble(binding.MAP_SURF), lambda: h.map_keyposes(),
               lambda: h.map_get_stamps(0, 0), lambda: h.map_set_stamps(0, [0.0]), lambda: h.map_set_keyposes(0, np.zeros((1, 6), F32)),
               lambda: h.loop_search([0]), lambda: h.graph_status(), lambda: h.graph_get_edges(), lambda: h.graph_optimize([0]),
               lambda: h.graph_get_estimate(0, 0), lambda: h.graph_set_edges(0, [-1], [0], [np.eye(3, 4)], [np.ones(6)]),
               lambda: h.graph_add_edge(0, 1, np.eye(3, 4), np.ones(6)), lambda: h.graph_add_loops([0], [dict(status=2, latest_id=1, closest_id=0, fitness=0.1, noise_variance=0.1, T=np.eye(4), between=np.eye(3, 4))]),
               lambda: h.lm_add_keyframe(*fr[0]), lambda: h.lm_set_keypose(0, fr[0][0]), lambda: h.lm_reset_window(), lambda: h.lm_get_keyframe(),
               lambda: h.dist_init(0, 1, bytes(binding.DIST_ID_BYTES)), lambda: h.set_option("ALEGO_MAP_MERGE", 0)):
        refused(fn)
    h.replay_create(1, 4)
    refused(lambda: h.stream_setup(0))
    # what keeps working
    assert h.lm_keyframe_count() == 0
    h.set_lm_params(np.zeros(6))
    h.lm_apply_correction(_rc([0.1, 0, 0]))
    h.trajectory_enable(8)
    for k in range(4):
        h.scan_process(_scan(k), stages=7)
    assert h.loc_status()["frames"] == 4 and h.loc_status()["window"] > 0
    assert len(h.lm_local_map()[1]) > 0 and len(h.trajectory()) == 4
    h.close()
    # too late / wrong kind of handle
    h = binding.Handle(p)
    h.scan_process(_scan(0), stages=7)
    refused(lambda: h.loc_enable(fr, 0.0))
    h.close()
    h = binding.Handle(p)
    h.map_enable(16, 1 << 16)
    refused(lambda: h.loc_enable(fr, 0.0))
    h.graph_enable(4)
    refused(lambda: h.loc_enable(fr, 0.0))
    h.close()
    h = binding.Handle(p, n_slots=3)
    h.replay_create(1, 4)
    for k in range(4):
        h.replay_load(0, k, _scan(k))
    h.stream_setup(0)
    refused(lambda: h.loc_enable(fr, 0.0))
    h.close()
    # capacity: a frame larger than the handle's key-frame clouds, with a message that names it
    h = binding.Handle(p)
    big = np.zeros((h.N + 1, 4), F32)
    refused(lambda: h.loc_enable(fr[:2] + [(fr[0][0], fr[0][1], big, fr[0][3])], 0.0), binding.ERR_CAPACITY, "frame 2")
    h.loc_enable(fr, 0.0)   # the refused call left the handle as it was
    assert h.loc_status()["frames"] == 4
    h.close()


@pytest.mark.gpu
def test_every_way_of_feeding_scans_localises_alike(lap_map):
    """alego_scan_process, alego_lo_process + alego_lm_process behind alego_ip_process, and alego_batch_run on host-loaded scans (no bag store)
    at sync 1 and sync 0: the same scans through the same kernels, so the LaserMapping state agrees bit for bit after every scan."""
    fr = [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in lap_map["frames"]]
    pl = _params(10)
    hs = [binding.Handle(pl) for _ in range(4)]
    for h in hs:
        h.loc_enable(fr, 6.0)
    ran = 0
    for k in range(30):
        pts = _scan(k)
        hs[0].scan_process(pts, stages=7)
        seg = hs[1].ip_process(pts)
        flags, feat, odom = hs[1].lo_process(seg)
        if k > 0:   # (the first scan only initialises LaserOdometry: no /odom/lidar, no mapping frame)
            fl, _ = hs[1].lm_process(feat["less_sharp"], feat["less_flat"], seg["outlier"], odom)
            assert not fl & binding.FLAG_LM_KEYFRAME
        for h, sync in ((hs[2], True), (hs[3], False)):
            h.batch_load(0, 0, pts)
            h.batch_run(0, 1, stages=7, sync=sync)
            h.synchronize()
        want = hs[0].debug_get("lm_state")
        ran += int(hs[0].debug_get("lm_info")[LI_RUN])
        for i, h in enumerate(hs[1:], 1):
            assert_bit_equal(h.debug_get("lm_state")[0:27], want[0:27], f"scan {k} path {i} lm_state")
            assert_bit_equal(h.debug_get("lm_state")[LD_LOC_P:LD_LOC_P + 3], want[LD_LOC_P:LD_LOC_P + 3], f"scan {k} path {i} p")
            assert_bit_equal(h.debug_get("lm_window"), hs[0].debug_get("lm_window"), f"scan {k} path {i} window")
            assert h.lm_keyframe_count() == 0
    assert ran >= 14 and hs[0].loc_status()["optimized"] == 1 and hs[0].loc_status()["rebuilds"] >= 2
    for i, h in enumerate(hs[1:], 1):
        assert h.loc_status() == hs[0].loc_status(), i
        for name in ("lm_corner_map_ds", "lm_surf_map_ds"):
            assert_bit_equal(h.debug_get(name), hs[0].debug_get(name), f"path {i} {name}")
    for h in hs:
        h.close()


@pytest.mark.gpu
def test_cpp_example_localises_in_its_own_map():
    exe = os.path.join(ROOT, "examples", "replay")
    r = subprocess.run([exe, "200", "--localize"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert np.isfinite(js["loc_max_dev"]) and js["loc_max_dev"] < 0.1, js
    # the same two runs through the binding
    p = _params()
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    track = []
    for k in range(200):
        flags, odom, mp = h.scan_process(_scan(k), stages=7, stamp=0.1 * k)
        track.append(mp["t"].copy())
    frames = [h.map_get_keyframe(i) for i in range(h.map_status()[0])]
    h.close()
    assert js["loc_frames"] == len(frames)
    h = binding.Handle(p)
    h.loc_enable([(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames], 0.0)
    dev = 0.0
    for k in range(200):
        flags, odom, mp = h.scan_process(_scan(k), stages=7, stamp=0.1 * k)
        dev = max(dev, np.abs(mp["t"] - track[k]).max())
    h.close()
    assert [float(v) for v in mp["t"]] == js["loc_map_t"], (mp["t"], js["loc_map_t"])
    assert float(f"{dev:.9g}") == js["loc_max_dev"], (dev, js["loc_max_dev"])
