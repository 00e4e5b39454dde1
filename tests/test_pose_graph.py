"""The key-pose graph (alego_graph_*, kernels_graph.hip, csrc/pg_math.h) against tests/pose_graph_ref.py, a numpy /
scipy restatement of the objective that shares no code with the library.  The restatement is checked first (central differences,
scipy.optimize.least_squares); then the host-only alego_graph_residuals; then, on the GPU, the recorded chain, the optimum of the lap's and
of constructed graphs, and the device's correctPoses against the existing per-slot calls, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_graph_ref as R
from alego_amd import binding, synth
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_graph_enable", "alego_graph_status", "alego_graph_get_edges", "alego_graph_set_edges", "alego_graph_add_loops", "alego_graph_add_edge",
               "alego_graph_optimize", "alego_graph_get_estimate", "alego_graph_residuals"]
F32 = np.float32
# Bound on |device estimate - restatement's optimum|: ten times the largest difference measured on the MI355X over every case of this file
# (lap, constructed graphs at step_tol 1e-10 and with the defaults, 64 loop edges): 2.7e-11 m in translation and
# 8.8e-13 rad in the rotation vector, both from the defaults' runs, whose last step stays just below 1e-9.  The cap would be 1e-6.
TOL_T, TOL_R = 2.7e-10, 8.8e-12
I34 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_graph_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in binding.EXPORTS, s
    assert (binding.GRAPH_MAX_ITERS, binding.GRAPH_STEP_TOL) == (int(re.search(r"#define ALEGO_GRAPH_MAX_ITERS (\d+)", hdr).group(1)),
                                                                 float(re.search(r"#define ALEGO_GRAPH_STEP_TOL (\S+)", hdr).group(1)))
    assert C.sizeof(binding.GraphEdge) == 152 and binding.GRAPH_MAX_LOOPS == int(re.search(r"#define ALEGO_GRAPH_MAX_LOOPS (\d+)", hdr).group(1))


def _rand_pose(rng, n, ang, tr):
    """n poses whose rotation angle is exactly `ang` (random axes) and whose tangent translation components have a magnitude in
    [0.3 tr, tr] and a random sign"""
    w = rng.normal(size=(n, 3))
    w *= (ang / np.linalg.norm(w, axis=1))[:, None]
    return R.exp_se3(np.concatenate([w, rng.uniform(0.3 * tr, tr, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))], 1))


def _random_graph(rng, n_poses, n_loops, err_angle, rel_t, var_lo=-8, var_hi=0):
    """a chain with a prior + random loop edges: positions in a box of side rel_t (so relative poses reach rel_t), ERROR transforms
    measured^-1 (x_from^-1 x_to) of rotation angle `err_angle` and of translations of the poses' own size — an error much smaller than the
    poses it is the difference of carries their rounding, 1e-16 |pose| / |error|, whatever the implementation"""
    X = _rand_pose(rng, n_poses, 1.0, 1.0)
    X[:, :, 3] = rng.uniform(-0.5 * rel_t, 0.5 * rel_t, (n_poses, 3))
    frm = list(range(-1, n_poses - 1))
    to = list(range(n_poses))
    for _ in range(n_loops if n_poses > 1 else 0):
        a, b = rng.choice(n_poses, 2, replace=False)
        frm.append(int(a)); to.append(int(b))
    frm, to = np.array(frm), np.array(to)
    h = R.between(X[np.maximum(frm, 0)], X[to])
    h[frm < 0] = X[to[frm < 0]]
    E = _rand_pose(rng, len(frm), err_angle, rel_t)
    meas = R.compose(h, R.between(E, np.tile(I34, (len(frm), 1, 1))))   # measured = h E^-1
    var = 10.0 ** rng.uniform(var_lo, var_hi, (len(frm), 6))
    return X, R.Graph(frm, to, meas, var)


def _numeric_jacobian(g, X, h=1e-6):
    n = len(X)
    J = np.zeros((6 * len(g.to), 6 * n))
    for k in range(6 * n):
        d = np.zeros(6 * n); d[k] = h
        rp = g.residuals(R.compose(X, R.exp_se3(d.reshape(n, 6)))).ravel()
        rm = g.residuals(R.compose(X, R.exp_se3(-d.reshape(n, 6)))).ravel()
        J[:, k] = (rp - rm) / (2 * h)
    return J


@pytest.mark.parametrize("angle", [1e-9, 1e-3, 0.0999, 0.1001, 1.0, 2.0, 2.2, np.pi - 1e-3])
def test_restatement_jacobians_match_central_differences(angle):
    rng = np.random.default_rng(3)
    X, g = _random_graph(rng, 6, 3, angle, 10.0)
    _, J = g.jacobian(X)
    Jn = _numeric_jacobian(g, X)
    # central differences with h = 1e-6 carry ~1e-10 of the largest entry (rounding / h); the blocks hold 1/sigma up to 1e4
    assert np.abs(J.toarray() - Jn).max() <= 2e-9 * np.abs(Jn).max()
    xi = R.log_se3(_rand_pose(rng, 50, angle, 5.0))
    assert np.abs(R.log_se3(R.exp_se3(xi)) - xi).max() < 1e-13 * 5


def drifted_circle(n, drift, seed=0, loops=((-1, 2),), loop_var=0.1):
    """the prototype's case: a circle of circumference ~n m driven once, odometry measurements with noise and bias scaled by `drift`,
    dead-reckoned initial poses, loop edges (from, to) (negative ids count from the end) measured at the TRUE relative pose.
    Returns (X0 dead-reckoned (n, 3, 4), Graph, true poses)."""
    rng = np.random.default_rng(seed)
    rad = max(n, 8) / (2 * np.pi)
    ang = np.arange(n) / max(n, 8) * 2 * np.pi * 0.985
    Xt = np.zeros((n, 3, 4))
    for i, a in enumerate(ang):
        T = R.exp_se3(np.array([0, 0, 0, rad * np.cos(a), rad * np.sin(a), 0.0]))
        T = R.compose(T, R.exp_se3(np.array([0, 0, a + np.pi / 2, 0, 0, 0])))
        Xt[i] = R.compose(T, R.exp_se3(np.array([0.02 * np.sin(3 * a), 0.02 * np.cos(2 * a), 0, 0, 0, 0])))
    rel = R.between(Xt[:-1], Xt[1:])
    noise = rng.normal(size=(n - 1, 6)) * np.array([2e-3, 2e-3, 2e-3, 1e-2, 1e-2, 1e-2]) * drift + np.array([0, 0, 1e-3, 0, 0, 2e-3]) * drift
    Zo = R.compose(rel, R.exp_se3(noise))
    X0 = np.zeros_like(Xt)
    X0[0] = Xt[0]
    for i in range(1, n):
        X0[i] = R.compose(X0[i - 1], Zo[i - 1])
    # the device starts from the f32 key poses: so does the graph's prior and the initial estimate
    X0 = R.from_pose6(R.to_pose6(X0))
    frm = list(range(-1, n - 1)); to = list(range(n))
    meas = [X0[0]] + list(Zo)
    var = [R.ODOM_VARIANCE] * n
    for a, b in loops:
        a, b = a % n, b % n
        frm.append(a); to.append(b); meas.append(R.between(Xt[a], Xt[b])); var.append(np.full(6, loop_var))
    return X0, R.Graph(frm, to, np.array(meas), np.array(var)), Xt


@pytest.mark.parametrize("n", [2, 3, 8, 30])
def test_restatement_optimum_matches_scipy_least_squares(n):
    from scipy.optimize import least_squares
    X0, g, _ = drifted_circle(n, 1.0, seed=n, loops=((-1, 0),), loop_var=0.01)
    X, steps, costs = g.optimize(X0)
    assert steps[-1] < 1e-12, steps
    fun = lambda d: g.residuals(R.compose(X0, R.exp_se3(d.reshape(n, 6)))).ravel()
    sol = least_squares(fun, np.zeros(6 * n), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1e-3, max_nfev=400)
    Xs = R.compose(X0, R.exp_se3(sol.x.reshape(n, 6)))
    # least_squares stops on its own tolerances with finite-difference Jacobians: ~1e-8 of the solution
    assert np.abs(Xs - X).max() < 1e-6, np.abs(Xs - X).max()
    assert abs(2 * sol.cost - costs[-1]) <= 1e-6 * max(1.0, costs[-1])
    assert costs[-1] <= costs[0]


def test_restatement_chain_without_loops_returns_its_input():
    X0, g, _ = drifted_circle(40, 1.0, loops=())
    g = R.Graph(*R.chain_graph(X0))
    X, steps, costs = g.optimize(X0)
    assert costs[0] < 1e-12 and costs[-1] < 1e-12, costs
    assert np.abs(X - X0).max() < 1e-12


def _compare_blocks(tag, got, want):
    for i in range(len(want)):
        scale = np.abs(want[i]).max()
        assert np.abs(got[i] - want[i]).max() <= 1e-12 * max(scale, 1e-300), (tag, i, np.abs(got[i] - want[i]).max() / max(scale, 1e-300))


RES_CASES = {   # error rotation angle, relative translations up to, tag
    "zero": (0.0, 10.0), "tiny": (1e-12, 10.0), "log_switch_below": (0.9e-10, 1.0), "log_switch_above": (1.1e-10, 1.0),
    "small": (1e-4, 100.0), "series_below": (0.1 * (1 - 1e-9), 100.0), "series_above": (0.1 * (1 + 1e-9), 100.0),
    "mid": (1.3, 100.0), "axis_switch_below": (2 * np.pi / 3 - 1e-9, 100.0), "axis_switch_above": (2 * np.pi / 3 + 1e-9, 100.0),
    "large": (3.0, 100.0), "near_pi": (np.pi - 1e-3, 100.0),
}


@pytest.mark.parametrize("case", sorted(RES_CASES))
def test_graph_residuals_match_restatement(case):
    angle, rel_t = RES_CASES[case]
    rng = np.random.default_rng(sorted(RES_CASES).index(case))
    for trial in range(20):
        X, g = _random_graph(rng, 12, 8, angle, rel_t if trial % 2 else 0.1 * rel_t)
        r, jf, jt = binding.graph_residuals(X, g.frm, g.to, g.meas, g.var)
        rw, jfw, jtw = g.linearize(X)
        _compare_blocks((case, trial, "residual"), r, rw)
        _compare_blocks((case, trial, "jac_from"), jf[g.frm >= 0], jfw[g.frm >= 0])
        _compare_blocks((case, trial, "jac_to"), jt, jtw)
        assert not jf[g.frm < 0].any()


def test_graph_residuals_argument_errors():
    L = binding.lib()
    X = np.tile(I34, (3, 1, 1)).reshape(3, 12).copy()
    ok = dict(frm=[0], to=[1], between=[I34], variance=[np.ones(6)])
    e = binding.graph_edges(**ok)
    out = np.zeros(36)
    assert L.alego_graph_residuals(X.ctypes.data, 3, e, 1, out.ctypes.data, None, None) == 0
    assert L.alego_graph_residuals(None, 3, e, 1, out.ctypes.data, None, None) == binding.ERR_ARG
    assert L.alego_graph_residuals(X.ctypes.data, 0, e, 1, out.ctypes.data, None, None) == binding.ERR_ARG
    assert L.alego_graph_residuals(X.ctypes.data, 3, None, 1, out.ctypes.data, None, None) == binding.ERR_ARG
    bad_b = I34.copy(); bad_b[0, 3] = np.nan
    for kw in (dict(frm=[1], to=[1]), dict(frm=[0], to=[3]), dict(frm=[-2], to=[1]), dict(frm=[3], to=[1]), dict(to=[-1]),
               dict(variance=[np.array([1, 1, 0, 1, 1, 1.0])]), dict(variance=[np.array([1, 1, -1, 1, 1, 1.0])]),
               dict(variance=[np.array([1, 1, np.inf, 1, 1, 1.0])]), dict(variance=[np.array([1, 1, np.nan, 1, 1, 1.0])]), dict(between=[bad_b])):
        e = binding.graph_edges(**{**ok, **kw})
        assert L.alego_graph_residuals(X.ctypes.data, 3, e, 1, out.ctypes.data, None, None) == binding.ERR_ARG, kw
    Xn = X.copy(); Xn[2, 5] = np.inf
    assert L.alego_graph_residuals(Xn.ctypes.data, 3, binding.graph_edges(**ok), 1, out.ctypes.data, None, None) == binding.ERR_ARG


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _lap():
    import test_loop_search as T
    return T


def _replay(p, starts, steps, graph, max_loops=4, max_frames=256, max_points=1 << 19):
    """the lap fixture's recipe (test_loop_search.replay_handle) with the graph enabled between alego_map_enable and the first scan"""
    T = _lap()
    h = binding.Handle(p, n_slots=len(starts))
    h.replay_create(1, T.LAP)
    for k in range(T.LAP):
        h.replay_load(0, k, T._scan(p, k))
    for s, st in enumerate(starts):
        h.replay_assign(s, 0, st)
    h.map_enable(max_frames, max_points)
    if graph:
        h.graph_enable(max_loops)
    h.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=False)
    h.synchronize()
    return h


def _archived_poses(h, slot):
    nf = h.map_status(slot)[0]
    return np.array([h.map_get_keyframe(j, slot=slot)["pose"] for j in range(nf)], F32).reshape(-1, 6)


def _graph_of(h, slot):
    c, l = h.graph_get_edges(0, slot=slot), h.graph_get_edges(1, slot=slot)
    return R.Graph(np.concatenate([c["frm"], l["frm"]]), np.concatenate([c["to"], l["to"]]), np.concatenate([c["between"], l["between"]]),
                   np.concatenate([c["variance"], l["variance"]]))


def _estimate_error(est, want):
    """largest |translation difference| (m) and largest |rotation-vector component| of want^-1 est (rad)"""
    d = R.log_se3(R.between(want, est))
    return float(np.abs(est[:, :, 3] - want[:, :, 3]).max()), float(np.abs(d[:, :3]).max())


STEPS = 420


@pytest.fixture(scope="module")
def lap():
    T = _lap()
    p = T._params(False)
    starts = [T.START(s) for s in range(T.N_SLOTS)]
    h = _replay(p, starts, STEPS, True)
    groups, per = h.stream_groups()
    assert groups >= 2
    sample = sorted({s for g in range(groups) for s in (g * per, min(T.N_SLOTS, (g + 1) * per) - 1)} | {37, 90})
    yield dict(p=p, h=h, starts=starts, sample=sample, n=T.N_SLOTS)
    h.close()


@pytest.mark.gpu
def test_recorded_chain_and_feature_off(lap):
    h, p, n = lap["h"], lap["p"], lap["n"]
    for s in lap["sample"]:
        poses = _archived_poses(h, s)
        want = R.Graph(*R.chain_graph(R.from_pose6(poses)))
        got = h.graph_get_edges(0, slot=s)
        assert len(poses) >= 10
        assert (got["frm"] == want.frm).all() and (got["to"] == want.to).all()
        assert np.abs(got["between"] - want.meas).max() <= 1e-12, (s, np.abs(got["between"] - want.meas).max())
        assert_bit_equal(got["variance"], np.tile(R.ODOM_VARIANCE, (len(poses), 1)), f"slot {s}: odometry variances")
    res = h.graph_optimize(list(range(n)))
    for s in lap["sample"]:
        X0 = R.from_pose6(_archived_poses(h, s))
        r = res[s]
        print(f"no-loop slot {s}: {r}")
        assert (r["status"], r["applied"], r["n_loops"], r["n_poses"]) == (2, 0, 0, len(X0)), r
        assert r["cost0"] < 1e-12 and r["cost"] < 1e-12, r   # (whitened f64 rounding of a pose of |t| ~ 30 m: 1e-14 / 1e-4)^2 per term
        et, er = _estimate_error(h.graph_get_estimate(slot=s), X0)
        assert et < 1e-12 and er < 1e-13, (s, et, er)
    # the same replay without alego_graph_enable: poses, archives and the loop search bit for bit
    off = _replay(p, lap["starts"], STEPS, False)
    try:
        with pytest.raises(binding.AlegoError):
            off.graph_optimize([0])
        a, b = h.loop_search(list(range(n))), off.loop_search(list(range(n)))
        for s in range(n):
            for k in a[s]:
                assert_bit_equal(np.asarray(a[s][k]), np.asarray(b[s][k]), f"slot {s}: loop search {k}")
            _, o1, m1 = h.batch_get_pose(s)
            _, o2, m2 = off.batch_get_pose(s)
            for k in ("t", "q"):
                assert_bit_equal(o1[k], o2[k], f"slot {s}: odom {k}")
                assert_bit_equal(m1[k], m2[k], f"slot {s}: map {k}")
            assert h.map_status(s) == off.map_status(s)
        for s in lap["sample"]:
            assert_bit_equal(_archived_poses(h, s), _archived_poses(off, s), f"slot {s}: archived poses")
            assert_bit_equal(h.map_assemble(7, slot=s), off.map_assemble(7, slot=s), f"slot {s}: global map")
    finally:
        off.close()


@pytest.fixture(scope="module")
def lap_closed():
    """a second replay of the same recipe for the tests that add loop edges (the `lap` handle stays without any)"""
    T = _lap()
    p = T._params(False)
    h = _replay(p, [T.START(s) for s in range(T.N_SLOTS)], STEPS, True)
    groups, per = h.stream_groups()
    sample = sorted({s for g in range(groups) for s in (g * per, min(T.N_SLOTS, (g + 1) * per) - 1)} | {37, 90})
    yield dict(h=h, sample=sample, n=T.N_SLOTS)
    h.close()


@pytest.mark.gpu
def test_lap_end_to_end(lap_closed):
    lap = lap_closed
    h, n = lap["h"], lap["n"]
    slots = list(range(n))
    found = h.loop_search(slots)
    h.graph_add_loops(slots, found)
    res = h.graph_optimize(slots)
    est = {s: h.graph_get_estimate(slot=s) for s in slots}
    closed = [s for s in lap["sample"] if found[s]["status"] == 2]
    assert closed, [found[s]["status"] for s in lap["sample"]]
    for s in lap["sample"]:
        r = res[s]
        assert r["status"] == 2 and r["applied"] == 0 and r["n_loops"] == (1 if found[s]["status"] == 2 else 0), r
        assert r["cost"] <= r["cost0"], r
        g = _graph_of(h, s)
        X0 = R.from_pose6(_archived_poses(h, s))
        want, steps, costs = g.optimize(X0)
        assert steps[-1] < 1e-9, steps
        et, er = _estimate_error(est[s], want)
        print(f"lap slot {s}: loops {r['n_loops']} iterations {r['iterations']} last_step {r['last_step']:.3e} cost {r['cost0']:.6e} -> {r['cost']:.6e} "
              f"(restatement {costs[0]:.6e} -> {costs[-1]:.6e}, steps {steps}) |dt| {et:.3e} m |dr| {er:.3e} rad moved {np.abs(want[:, :, 3] - X0[:, :, 3]).max():.3e} m")
        assert et <= TOL_T and er <= TOL_R, (s, et, er)
        assert abs(r["cost"] - costs[-1]) <= 1e-9 * max(1.0, costs[-1]) and abs(r["cost0"] - costs[0]) <= 1e-9 * max(1.0, costs[0])
    # a slot's result does not depend on the company it is optimised in: alone, reversed, chunked
    rev = h.graph_optimize(slots[::-1])[::-1]
    for s in slots:
        for k in res[s]:
            assert_bit_equal(np.asarray(rev[s][k]), np.asarray(res[s][k]), f"slot {s} reversed: {k}")
        assert_bit_equal(h.graph_get_estimate(slot=s), est[s], f"slot {s} reversed: estimate")
    for s in (0, 1, 63, 64, 127):
        one = h.graph_optimize([s])[0]
        for k in res[s]:
            assert_bit_equal(np.asarray(one[k]), np.asarray(res[s][k]), f"slot {s} alone: {k}")
        assert_bit_equal(h.graph_get_estimate(slot=s), est[s], f"slot {s} alone: estimate")
    h.set_option("ALEGO_PG_BUDGET", 3 << 20)   # chunks of a few slots
    small = h.graph_optimize(slots)
    h.set_option("ALEGO_PG_BUDGET", 1 << 30)
    for s in slots:
        for k in res[s]:
            assert_bit_equal(np.asarray(small[s][k]), np.asarray(res[s][k]), f"slot {s} chunked: {k}")
        assert_bit_equal(h.graph_get_estimate(slot=s), est[s], f"slot {s} chunked: estimate")


ONE = np.array([[1.0, 2.0, 0.5, 0.0]], F32)


def _constructed_handle(graphs, max_loops, max_frames):
    """one slot per (X0, Graph): frames inserted with alego_lm_add_keyframe at the dead-reckoned poses, the recorded chain overwritten with
    the graph's chain edges; loop edges are NOT added"""
    p = synth.default_params(16, 1800)
    h = binding.Handle(p, n_slots=len(graphs))
    h.map_enable(max_frames, 4 * max_frames)
    h.graph_enable(max_loops)
    for s, (X0, g) in enumerate(graphs):
        n = len(X0)
        for kp in R.to_pose6(X0):
            h.lm_reset_window(slot=s)
            h.lm_add_keyframe(kp, ONE, ONE, ONE, slot=s)
        n = min(n, h.map_status(s)[0])   # (an archive that is too small keeps a prefix)
        if n:
            h.graph_set_edges(0, g.frm[:n], g.to[:n], g.meas[:n], g.var[:n], slot=s)
    return h


def _add_loops(h, s, g, n):
    for i in range(n, len(g.to)):
        h.graph_add_edge(g.frm[i], g.to[i], g.meas[i], g.var[i], slot=s)


# The prototype's cases: 150 poses at 3.3 m / 0.15 rad and 5.5 m / 0.26 rad end drift, 400 poses at ~19 m / 0.27 rad; one noise seed, so the
# 150-pose cases differ in their loop edges only.  Every case asserts the end drift it claims, in metres and in radians.  Two deviations
# from "3 - 20 m / 0.15 - 0.35 rad", stated in DESIGN.md section 13: the generator's drift is a yaw bias, so over 2000 poses (a 318 m radius)
# 20 m of end drift leave 0.06 rad; and two or three poses one metre apart cannot drift by 3 m, so those two cases claim the rotation only.
BIG = ((3.0, 20.0), (0.15, 0.35))
CONSTRUCTED = {   # n poses, drift scale, loops (from, to), loop variance, correction meant to be > 1 m, claimed end drift ((m), (rad))
    "circle2": (2, 100.0, ((1, 0),), 0.1, False, ((0.5, 3.0), (0.15, 0.35))),
    "circle3": (3, 80.0, ((2, 0),), 0.1, False, ((0.5, 3.0), (0.15, 0.35))),
    "circle150": (150, 1.0, ((-1, 2),), 0.1, True, BIG),
    "circle150_drift": (150, 1.7, ((-1, 2),), 0.1, True, BIG),
    "circle150_tight": (150, 1.0, ((-1, 2),), 1e-4, True, BIG),
    "circle150_loose": (150, 2.2, ((-1, 2),), 0.4, True, BIG),
    "circle400": (400, 0.7, ((-1, 2),), 0.1, True, BIG),
    "two_loops_nested": (150, 1.0, ((-1, 2), (-30, 20)), 0.1, True, BIG),
    "crossing_and_duplicate": (150, 1.0, ((-1, 2), (100, 10), (-20, 60), (-1, 2)), 0.1, True, BIG),
    "neighbours": (150, 1.0, ((-1, 2), (41, 40), (40, 41)), 0.1, True, BIG),
    "max_loops": (150, 1.0, ((-1, 2), (-2, 3), (-3, 1), (-10, 5), (120, 30), (90, 60), (70, 0), (-1, 0)), 0.1, True, BIG),
    "circle2000": (2000, 0.028, ((-1, 2),), 0.1, True, ((3.0, 20.0), (0.05, 0.35))),
}
MAX_LOOPS = 8


@pytest.fixture(scope="module")
def constructed():
    names = sorted(CONSTRUCTED)
    graphs = []
    for k in names:
        n, drift, loops, lv = CONSTRUCTED[k][:4]
        X0, g, _ = drifted_circle(n, drift, loops=loops, loop_var=lv)
        graphs.append((X0, g))
    h = _constructed_handle(graphs, MAX_LOOPS, 2048)
    for s, (X0, g) in enumerate(graphs):
        _add_loops(h, s, g, len(X0))
    yield dict(h=h, names=names, graphs=graphs)
    h.close()


@pytest.mark.gpu
def test_constructed_graphs(constructed):
    h, names, graphs = constructed["h"], constructed["names"], constructed["graphs"]
    res = h.graph_optimize(list(range(len(names))), max_iters=50, step_tol=1e-10)
    worst = [0.0, 0.0]
    for s, k in enumerate(names):
        X0, g = graphs[s]
        n = len(X0)
        # the premise, on the restatement: Gauss-Newton converges, and the correction is large where the case is meant to be
        want, steps, costs = g.optimize(X0)
        moved = float(np.abs(want[:, :, 3] - X0[:, :, 3]).max())
        Xt = constructed_truth(k)
        end = float(np.linalg.norm(X0[-1, :, 3] - Xt[-1, :, 3]))
        rot = float(np.linalg.norm(R.log_se3(R.between(Xt[-1:], X0[-1:]))[0, :3]))
        (lo_m, hi_m), (lo_r, hi_r) = CONSTRUCTED[k][5]
        assert steps[-1] < 1e-10, (k, steps)
        assert lo_m <= end <= hi_m and lo_r <= rot <= hi_r, (k, end, rot)
        if CONSTRUCTED[k][4]:
            assert moved > 1.0, (k, moved)
        r = res[s]
        got = h.graph_get_edges(0, slot=s)
        assert np.array_equal(got["between"], g.meas[:n]) and len(h.graph_get_edges(1, slot=s)["to"]) == len(g.to) - n
        est = h.graph_get_estimate(slot=s)
        et, er = _estimate_error(est, want)
        worst = [max(worst[0], et), max(worst[1], er)]
        n_to_1e4 = 1 + next(i for i, v in enumerate(steps) if v < 1e-4)
        print(f"constructed {k}: n {n} loops {r['n_loops']} end drift {end:.2f} m {rot:.3f} rad moved {moved:.2f} m device iterations {r['iterations']} last_step {r['last_step']:.3e} "
              f"cost {r['cost0']:.6e} -> {r['cost']:.6e}; restatement {len(steps)} steps ({n_to_1e4} to 1e-4) {['%.1e' % v for v in steps]} cost {costs[0]:.6e} -> {costs[-1]:.6e}; "
              f"|dt| {et:.3e} m |dr| {er:.3e} rad")
        assert (r["status"], r["n_poses"], r["n_loops"], r["applied"]) == (2, n, len(g.to) - n, 0), (k, r)
        assert r["cost"] <= r["cost0"], (k, r)
        assert abs(r["cost"] - costs[-1]) <= 1e-9 * max(1.0, costs[-1]), (k, r["cost"], costs[-1])
        assert et <= TOL_T and er <= TOL_R, (k, et, er)
    print(f"constructed: largest |dt| {worst[0]:.3e} m, largest |dr| {worst[1]:.3e} rad")
    # the defaults reach the same optimum
    dflt = h.graph_optimize(list(range(len(names))))
    for s, k in enumerate(names):
        want, _, _ = graphs[s][1].optimize(graphs[s][0])
        et, er = _estimate_error(h.graph_get_estimate(slot=s), want)
        print(f"constructed {k} with the defaults: iterations {dflt[s]['iterations']} last_step {dflt[s]['last_step']:.3e} |dt| {et:.3e} |dr| {er:.3e}")
        assert dflt[s]["status"] == 2 and et <= TOL_T and er <= TOL_R, (k, dflt[s], et, er)
        assert dflt[s]["iterations"] <= binding.GRAPH_MAX_ITERS // 2, (k, dflt[s])   # max_iters is twice the worst case
    # where the steps stagnate (the level step_tol has to stay 100 x above): 30 steps with a tolerance that is never met
    stag = h.graph_optimize(list(range(len(names))), max_iters=30, step_tol=1e-300)
    for s, k in enumerate(names):
        print(f"constructed {k} stagnation: status {stag[s]['status']} iterations {stag[s]['iterations']} last_step {stag[s]['last_step']:.3e}")
        assert stag[s]["status"] in (1, 2) and stag[s]["last_step"] < 1e-2 * binding.GRAPH_STEP_TOL, (k, stag[s])
    # max_iters = 1: a drifted loop is not converged after one step and nothing is applied
    s = names.index("circle150")
    before = _archived_poses(h, s)
    one = h.graph_optimize([s], max_iters=1, apply=True)[0]
    assert (one["status"], one["iterations"], one["applied"]) == (1, 1, 0), one
    assert_bit_equal(_archived_poses(h, s), before, "max_iters = 1 leaves the archive alone")
    # a full max_loops: capacity error, graph unchanged
    s = names.index("max_loops")
    g = graphs[s][1]
    loops = h.graph_get_edges(1, slot=s)
    assert len(loops["to"]) == MAX_LOOPS
    with pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_CAPACITY}\)"):
        h.graph_add_edge(5, 50, I34, np.full(6, 0.1), slot=s)
    again = h.graph_get_edges(1, slot=s)
    for key in loops:
        assert_bit_equal(again[key], loops[key], f"loop edges after the capacity error: {key}")


def constructed_truth(k):
    n, drift, loops, lv = CONSTRUCTED[k][:4]
    return drifted_circle(n, drift, loops=loops, loop_var=lv)[2]


@pytest.mark.gpu
def test_sixty_four_loop_edges():
    """ALEGO_GRAPH_MAX_LOOPS loop edges: 385 right-hand sides sweep on seven wavefronts and the capacitance system is 384 x 384"""
    rng = np.random.default_rng(64)
    loops = [(-1, 2)]
    while len(loops) < binding.GRAPH_MAX_LOOPS:
        a, b = (int(v) for v in rng.choice(150, 2, replace=False))
        loops.append((a, b))
    X0, g, Xt = drifted_circle(150, 1.0, loops=tuple(loops), loop_var=0.1)
    g.var[150:] = 10.0 ** rng.uniform(-4, np.log10(0.4), (len(loops), 1))
    g = R.Graph(g.frm, g.to, g.meas, g.var)
    want, steps, costs = g.optimize(X0)
    assert steps[-1] < 1e-10 and np.abs(want[:, :, 3] - X0[:, :, 3]).max() > 1.0, steps
    h = _constructed_handle([(X0, g)], binding.GRAPH_MAX_LOOPS, 256)
    try:
        _add_loops(h, 0, g, 150)
        assert h.graph_status(0)[:3] == (150, 64, 1)
        r = h.graph_optimize([0], max_iters=50, step_tol=1e-10)[0]
        et, er = _estimate_error(h.graph_get_estimate(slot=0), want)
        print(f"constructed 64 loops: device iterations {r['iterations']} last_step {r['last_step']:.3e} cost {r['cost0']:.6e} -> {r['cost']:.6e}; "
              f"restatement {['%.1e' % v for v in steps]} cost {costs[0]:.6e} -> {costs[-1]:.6e}; |dt| {et:.3e} m |dr| {er:.3e} rad")
        assert (r["status"], r["n_poses"], r["n_loops"]) == (2, 150, 64), r
        assert r["cost"] <= r["cost0"] and abs(r["cost"] - costs[-1]) <= 1e-9 * max(1.0, costs[-1]), (r, costs[-1])
        assert et <= TOL_T and er <= TOL_R, (et, er)
        again = h.graph_optimize([0], max_iters=50, step_tol=1e-10)[0]
        for k in r:
            assert_bit_equal(np.asarray(again[k]), np.asarray(r[k]), f"64 loops, repeated: {k}")
    finally:
        h.close()


@pytest.mark.gpu
def test_single_frame_no_frame_and_dropped_frames():
    X1, g1, _ = drifted_circle(1, 1.0, loops=())
    X5, g5, _ = drifted_circle(5, 1.0, loops=())
    h = _constructed_handle([(X1, g1), (X1[:0], g1), (X5, g5)], 2, 3)   # slot 2: 5 frames into an archive of 3
    try:
        r = h.graph_optimize([0, 1, 2])
        assert (r[0]["status"], r[0]["n_poses"], r[0]["iterations"]) == (2, 1, 1) and r[0]["cost0"] < 1e-12, r[0]
        et, er = _estimate_error(h.graph_get_estimate(slot=0), X1)
        assert et < 1e-12 and er < 1e-13
        assert (r[1]["status"], r[1]["n_poses"]) == (0, 0), r[1]
        assert h.map_status(2)[:2] == (3, 2) and r[2]["status"] == -1, (h.map_status(2), r[2])
    finally:
        h.close()


def _apply_by_hand(h, slot, est, correction, K):
    """the parent's way to apply a correction: the per-slot calls of INTEGRATION.md"""
    poses = R.to_pose6(est)
    n = len(poses)
    h.map_set_keyposes(0, poses, slot=slot)
    for kf in range(max(0, n - K), n):
        h.lm_set_keypose(kf, poses[kf], slot=slot)
    h.lm_reset_window(slot=slot)
    h.lm_apply_correction(np.asarray(correction, np.float64).reshape(4, 4)[:3, :], slot=slot)


@pytest.mark.gpu
def test_apply_equals_the_per_slot_calls():
    T = _lap()
    p = T._params(False)
    starts = [T.START(0), T.START(37), T.START(64)]
    A, B = _replay(p, starts, STEPS, True), _replay(p, starts, STEPS, True)
    try:
        slots = list(range(len(starts)))
        found = A.loop_search(slots)
        assert any(f["status"] == 2 for f in found), [f["status"] for f in found]
        # a large, known correction on top of the lap's small one: slot 0 also gets a loop edge that pulls its newest frame 2 m sideways
        n0 = A.map_status(0)[0]
        X = R.from_pose6(_archived_poses(A, 0))
        pull = R.compose(R.between(X[n0 - 1], X[3]), R.exp_se3(np.array([0, 0, 0.05, 0.5, 2.0, 0.1])))
        corr = np.eye(4, dtype=F32); corr[:3, :3] = R.exp_se3(np.array([0, 0, 0.02, 0, 0, 0]))[:, :3]; corr[:3, 3] = [0.3, -0.2, 0.05]
        for h in (A, B):
            h.graph_add_loops(slots, found)
            h.graph_add_edge(n0 - 1, 3, pull, np.full(6, 1e-4), correction=corr, slot=0)
        ra = A.graph_optimize(slots, apply=True)
        rb = B.graph_optimize(slots, apply=False)
        K = p.recent_keyframe_num
        for s in slots:
            closed = found[s]["status"] == 2 or s == 0
            assert ra[s]["status"] == 2 and ra[s]["applied"] == (1 if closed else 0), (s, ra[s])
            for k in ("status", "iterations", "cost0", "cost", "last_step"):
                assert ra[s][k] == rb[s][k], (s, k)
            est = A.graph_get_estimate(slot=s)
            assert_bit_equal(B.graph_get_estimate(slot=s), est, f"slot {s}: estimate")
            if closed:
                _apply_by_hand(B, s, est, corr if s == 0 else found[s]["T"], K)
        moved = np.abs(_archived_poses(A, 0)[:, :3] - R.to_pose6(X)[:, :3]).max()
        assert moved > 0.5, moved

        def same(tag):
            for s in slots:
                nf = A.map_status(s)[0]
                assert A.map_status(s) == B.map_status(s)
                assert_bit_equal(_archived_poses(A, s), _archived_poses(B, s), f"{tag} slot {s}: archived poses")
                for kf in range(max(0, nf - K), nf):
                    a, b = A.lm_get_keyframe(kf, slot=s), B.lm_get_keyframe(kf, slot=s)
                    for key in ("pose", "corner", "surf", "outlier"):
                        assert_bit_equal(a[key], b[key], f"{tag} slot {s} key frame {kf}: {key}")
                for name in ("lm_kf_corner_map", "lm_kf_surf_map", "lm_state"):
                    assert_bit_equal(A.debug_get(name, slot=s), B.debug_get(name, slot=s), f"{tag} slot {s}: {name}")
                assert_bit_equal(A.map_assemble(7, slot=s), B.map_assemble(7, slot=s), f"{tag} slot {s}: global map")
                (_, oa, ma), (_, ob, mb) = A.batch_get_pose(s), B.batch_get_pose(s)
                for key in ("t", "q"):
                    assert_bit_equal(oa[key], ob[key], f"{tag} slot {s}: odom {key}")
                    assert_bit_equal(ma[key], mb[key], f"{tag} slot {s}: map {key}")
        same("after apply")
        # a second optimise without a new loop edge applies nothing
        again = A.graph_optimize(slots, apply=True)
        assert [r["applied"] for r in again] == [0] * len(slots), again
        same("after the second optimise")
        for h in (A, B):
            h.batch_run(STEPS, 40, stages=7 | binding.REPLAY_BAG, sync=True)
        same("40 scans later")
        for s in slots:
            for a, b, name in zip(A.lm_local_map(slot=s), B.lm_local_map(slot=s), ("corner", "surf")):
                assert len(a) > 100
                assert_bit_equal(a, b, f"40 scans later slot {s}: local {name} map")
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_misuse():
    p = synth.default_params(16, 1800)
    h = binding.Handle(p, n_slots=2)
    err = lambda code: pytest.raises(binding.AlegoError, match=rf"\({code}\)")
    try:
        with err(binding.ERR_ARG):
            h.graph_enable(4)                      # before alego_map_enable
        h.map_enable(16, 64)
        with err(binding.ERR_ARG):
            h.graph_optimize([0])                  # graph off
        for bad in (0, binding.GRAPH_MAX_LOOPS + 1):
            with err(binding.ERR_ARG):
                h.graph_enable(bad)
        with err(binding.ERR_ARG):
            h.graph_enable(4, odom_variance=[1, 1, 1, 0, 1, 1])
        h.graph_enable(2)
        with err(binding.ERR_ARG):
            h.graph_enable(2)                      # twice
        X0, g, _ = drifted_circle(4, 1.0, loops=())
        for kp in R.to_pose6(X0):
            h.lm_reset_window(slot=0)
            h.lm_add_keyframe(kp, ONE, ONE, ONE, slot=0)
        v = np.full(6, 0.1)
        with err(binding.ERR_ARG):
            h.graph_optimize([0, 1, 0])            # a slot listed twice
        for slot in (-1, 2):
            with err(binding.ERR_ARG):
                h.graph_optimize([0, slot])
            with err(binding.ERR_ARG):
                h.graph_add_edge(0, 2, I34, v, slot=slot)
            with err(binding.ERR_ARG):
                h.graph_get_edges(0, 0, 1, slot=slot)
        nanb = I34.copy(); nanb[1, 1] = np.nan
        for frm, to, b, var in ((0, 4, I34, v), (4, 0, I34, v), (-1, 2, I34, v), (2, 2, I34, v), (0, 2, nanb, v), (0, 2, I34, v * 0), (0, 2, I34, -v),
                                (0, 2, I34, v * np.inf)):
            with err(binding.ERR_ARG):
                h.graph_add_edge(frm, to, b, var, slot=0)
        with err(binding.ERR_ARG):
            h.graph_add_edge(0, 1, I34, v, slot=1)   # slot 1 has no frames
        assert len(h.graph_get_edges(1, slot=0)["to"]) == 0
        with err(binding.ERR_ARG):
            h.graph_get_edges(0, 2, 3, slot=0)     # beyond the stored edges
        with err(binding.ERR_ARG):
            h.graph_get_edges(2, 0, 1, slot=0)     # no such kind
        c = h.graph_get_edges(0, slot=0)
        with err(binding.ERR_ARG):
            h.graph_set_edges(1, c["frm"][:2], c["to"][:2], c["between"][:2], c["variance"][:2], slot=0)   # edge ids do not match their place
        with err(binding.ERR_ARG):
            h.graph_set_edges(3, c["frm"][3:], c["to"][3:], c["between"][3:], c["variance"][3:] * 0, slot=0)
        with err(binding.ERR_ARG):
            h.graph_get_estimate(0, 1, slot=0)     # no optimise yet
        after = h.graph_get_edges(0, slot=0)
        for key in c:
            assert_bit_equal(after[key], c[key], f"chain after refused calls: {key}")
        r = h.graph_optimize([0])[0]
        assert r["status"] == 2 and r["n_poses"] == 4
        # a handle created after the first key frame cannot start a graph
        h2 = binding.Handle(p, n_slots=1)
        try:
            h2.map_enable(16, 64)
            h2.lm_add_keyframe(R.to_pose6(X0)[0], ONE, ONE, ONE)
            with err(binding.ERR_ARG):
                h2.graph_enable(2)
        finally:
            h2.close()
    finally:
        h.close()
