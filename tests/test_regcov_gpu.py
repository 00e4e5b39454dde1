"""-m gpu: lm_regcov (kernels_lm.hip) — the covariance of LaserMapping's scan-to-map registration and its degeneracy on the device (DESIGN.md
section 22), through alego_regcov_enable / alego_regcov_get / alego_debug_regcov and the odometry edges map_archive records.

Floating-point tolerances are measured, then asserted at 16 x (the margin covers the kernel's summation order — thread-strided partial sums
through block_reduce28 instead of row order — and the device's sin / cos).  Figures of the MI355X run, relative as in
tests/test_reg_cov_math.py (info to its largest entry, eigenvalues to lambda_max, cov and the variances to cov's largest entry, cost and sigma2 to
themselves):
                                                                   cost      info      eigenvalues  cov       sigma2
    kernel on given rows against the host twins (DEBUG_CASES)     8.48e-16  4.09e-15  2.54e-15     3.02e-14  8.28e-16
    mapping frames of the synthetic stream against numpy          1.79e-15  2.95e-15  2.62e-15     2.40e-14  1.87e-15
Integers, statuses and everything that is compared between two device runs are exact."""
import numpy as np
import pytest

import pose_graph_ref as R
import regcov_ref as ref
from alego_amd import binding
from test_reg_cov_math import deviations
from util import assert_bit_equal, assert_same_record, lm_observables as _observables, reg_params as _params, reg_rows_of_frame, reg_scan as _scan

F32 = np.float32
LI_NKF, LI_RUN, LI_FRAME, LI_FLAGS, LI_NCC, LI_NSC, LI_OPTIMIZED, LI_NCUR_C, LI_NTOTAL_DS, LI_REC_CNT = 0, 2, 4, 5, 6, 7, 11, 19, 23, 26
LD_PARAMS_IT = 27
# 16 x the largest deviation measured on the MI355X (acc: the cost alone here; the kernel does not return the normal equations)
TOL_TWIN = dict(acc=1.36e-14, info=6.54e-14, eigval=4.06e-14, cov=4.83e-13, sigma2=1.32e-14)
TOL_NUMPY = dict(acc=2.87e-14, info=4.72e-14, eigval=4.19e-14, cov=3.84e-13, sigma2=2.99e-14)
REC_FLOATS = ("cost", "sigma2", "info", "eigval", "eigvec", "cov", "variance")
REC_INTS = ("status", "n_edge", "n_plane", "n_degenerate", "frame")
ODOM_VAR = np.array([1e-4, 1e-4, 1e-4, 1e-3, 1e-3, 1e-3])   # of the graph tests: unlike any variance a registration yields
N_SCANS = 16


def _same_record(a, b, what):
    assert_same_record(a, b, what, REC_INTS, REC_FLOATS)


def _dev(got, want):
    """deviations() of two records (the cost in place of the normal equations)"""
    acc_g, acc_w = np.ones(28), np.ones(28)
    acc_g[27], acc_w[27] = got["cost"] if want["status"] == 1 else 1.0, want["cost"] if want["status"] == 1 else 1.0
    return deviations(acc_g, got, acc_w, want)


# ---- 3. the kernel alone on given rows against the host twins ----------------------------------------------------------------------
def _debug_cases():
    c = {}
    for n in (0, 6, 7, 255, 256, 257, 1000):   # LM_SOLVE_T = 256 threads stride over the queries
        c[f"edges_{n}"] = ref.courtyard(n_edge=n, n_plane=0, seed=100 + n)
        c[f"planes_{n}"] = ref.courtyard(n_edge=0, n_plane=n, seed=200 + n)
        c[f"mixed_{n}"] = ref.courtyard(n_edge=n // 2, n_plane=n - n // 2, seed=300 + n)
    c["corridor"] = ref.corridor()
    c["pitched_257"] = ref.courtyard(n_edge=100, n_plane=157, seed=9, p=np.array([-4.0, 2.0, 1.0, -0.4, 1.2, -3.0]))
    return c


DEBUG_CASES = _debug_cases()


@pytest.fixture(scope="module")
def plain_handle():
    h = binding.Handle(_params())
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEBUG_CASES))
def test_kernel_on_given_rows_against_the_host_twins(plain_handle, name):
    p, E, S = DEBUG_CASES[name]
    huber = plain_handle.params.huber_delta
    acc = binding.regcov_normal_host(p, E, S, huber)
    want = binding.regcov_host(acc, p, len(E), len(S))
    got = plain_handle.debug_regcov(p, E, S)
    for k in REC_INTS:
        assert got[k] == want[k], (name, k, got[k], want[k])
    assert got["status"] == (1 if len(E) + len(S) > 6 else 0)
    if name == "corridor":
        assert got["n_degenerate"] == 1 and abs(got["eigvec"][3, 0]) > 0.99
    f = _dev(got, want)
    print(f"{name}: kernel - host twin " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
    if got["status"] == 1:
        r, _ = ref.rows_jacobian(p, E, S)
        assert (np.abs(r) > huber).any() and (np.abs(r) < huber).any(), "rows on both sides of Huber's delta"
        assert np.array_equal(got["cov"], got["cov"].T) and np.array_equal(got["info"], got["info"].T)
    else:
        for k in REC_FLOATS:
            assert not np.any(got[k]), (name, k)
    for k, v in f.items():
        assert v <= TOL_TWIN[k], (name, k, v, TOL_TWIN[k])


@pytest.mark.gpu
def test_kernel_statuses(plain_handle):
    p, E, S = DEBUG_CASES["mixed_257"]
    up = p.copy(); up[4] = np.pi / 2
    assert plain_handle.debug_regcov(up, E, S)["status"] == -3
    bad = E.copy(); bad[5, 0] = np.nan
    r = plain_handle.debug_regcov(p, bad, S)
    assert r["status"] == -2 and (r["n_edge"], r["n_plane"]) == (len(E), len(S)) and not any(np.any(r[k]) for k in REC_FLOATS)
    nanp = p.copy(); nanp[0] = np.inf
    assert plain_handle.debug_regcov(nanp, E, S)["status"] == -2


# ---- 4. mapping frames of the synthetic stream, everything on (the run's archive is also the map of 8) -----------------------------
def _rows_of_frame(h, slot=0):
    """the accepted rows of the slot's last mapping frame as lm_fit left them, and the solver's final point"""
    gi, E, S = reg_rows_of_frame(h, slot)
    x = h.debug_get("lm_state", slot=slot)[LD_PARAMS_IT + 6:LD_PARAMS_IT + 12]
    return gi, x, E, S


def _slam_handle(graph, var_min=(1e-12,) * 6, n_slots=1):
    """archive + graph + the feature; var_min far below any variance a registration yields, so the clamp stays out of the way"""
    p = _params()
    assert p.lm_outer_iters == 2   # (_rows_of_frame reads the second row of LD_PARAMS_IT)
    h = binding.Handle(p, n_slots=n_slots)
    h.map_enable(64, 1 << 19)
    h.graph_enable(4, odom_variance=ODOM_VAR)
    h.regcov_enable(binding.regcov_opts(var_min=var_min, graph=graph))
    return h


@pytest.fixture(scope="module")
def stream_log():
    h = _slam_handle(1)
    log = []
    for k in range(N_SCANS):
        flags, odom, mp = h.scan_process(_scan(k), stages=7)
        gi, x, E, S = _rows_of_frame(h)
        log.append(dict(k=k, flags=flags, gi=gi, x=x, E=E, S=S, rec=h.regcov_get([0])[0], frames=h.map_status()[0]))
    yield h, log
    h.close()


@pytest.mark.gpu
def test_mapping_frames_against_numpy(stream_log):
    h, log = stream_log
    huber = h.params.huber_delta
    seen = 0
    worst = {k: 0.0 for k in TOL_NUMPY}
    last = None
    for e in log:
        gi, rec = e["gi"], e["rec"]
        if not gi[LI_RUN]:
            if last is not None:
                _same_record(rec, last, f"scan {e['k']}: a frame that does not map keeps the record")
            continue
        last = rec
        assert rec["frame"] == gi[LI_FRAME], (e["k"], rec["frame"], gi[LI_FRAME])
        if not gi[LI_OPTIMIZED]:
            assert gi[LI_FLAGS] & 16 and rec["status"] == 0 and (rec["n_edge"], rec["n_plane"]) == (0, 0), (e["k"], rec["status"])
            continue
        assert (rec["n_edge"], rec["n_plane"]) == (gi[LI_NCC], gi[LI_NSC]) == (len(e["E"]), len(e["S"])), e["k"]
        acc = ref.normal_equations(e["x"], e["E"], e["S"], huber)
        want = ref.record(acc, e["x"], len(e["E"]), len(e["S"]), var_min=np.full(6, 1e-12))
        assert rec["status"] == want["status"] == 1 and rec["n_degenerate"] == want["n_degenerate"], (e["k"], rec["status"], want["status"])
        f = _dev(rec, want)
        print(f"scan {e['k']}: {len(e['E'])} edges {len(e['S'])} planes, eigenvalues {rec['eigval'][0]:.3g} .. {rec['eigval'][5]:.3g}, n_degenerate {rec['n_degenerate']}; "
              "device - numpy " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
        worst = {k: max(worst[k], f[k]) for k in f}
        seen += 1
    print("largest over the frames: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert seen >= 5, seen
    for k, v in worst.items():
        assert v <= TOL_NUMPY[k], (k, v, TOL_NUMPY[k])


# ---- 5. nothing else moves -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_else_moves():
    p = _params()
    A, B = binding.Handle(p, n_slots=2), binding.Handle(p, n_slots=2)
    try:
        B.regcov_enable()
        for k in range(N_SCANS):
            for s in (0, 1):
                ra, rb = A.scan_process(_scan(k, s), stages=7, slot=s), B.scan_process(_scan(k, s), stages=7, slot=s)
                assert ra[0] == rb[0], (k, s, ra[0], rb[0])
                for i in (1, 2):
                    for key in ("t", "q", "params"):
                        assert_bit_equal(ra[i][key], rb[i][key], f"scan {k} slot {s}: pose {i} {key}")
            if k % 4 == 3:
                for s in (0, 1):
                    oa, ob = _observables(A, s), _observables(B, s)
                    for key in oa:
                        assert_bit_equal(oa[key], ob[key], f"scan {k} slot {s}: {key}")
        for s in (0, 1):
            assert A.lm_keyframe_count(s) == B.lm_keyframe_count(s) >= 5
            ka, kb = A.lm_get_keyframe(-1, slot=s), B.lm_get_keyframe(-1, slot=s)
            for key in ("pose", "corner", "surf", "outlier"):
                assert_bit_equal(ka[key], kb[key], f"slot {s}: newest key frame {key}")
        assert all(r["status"] == 1 for r in B.regcov_get([0, 1]))
    finally:
        A.close(); B.close()


# ---- 6. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_slot_does_not_depend_on_its_company():
    p = _params()
    H3 = binding.Handle(p, n_slots=3)
    singles = [binding.Handle(p) for _ in range(3)]
    try:
        H3.regcov_enable()
        for h in singles:
            h.regcov_enable()
        ones = 0
        for k in range(10):
            for s in range(3):
                H3.scan_process(_scan(k, s), stages=7, slot=s)
                singles[s].scan_process(_scan(k, s), stages=7)
            got = H3.regcov_get([2, 0, 1])
            for s, g in zip((2, 0, 1), got):
                _same_record(g, singles[s].regcov_get([0])[0], f"scan {k} slot {s}")
                ones += g["status"] == 1
        assert ones >= 9
        a, b = H3.regcov_get([0])[0], H3.regcov_get([1])[0]
        assert not np.array_equal(a["info"], b["info"]), "the streams differ"
    finally:
        H3.close()
        for h in singles:
            h.close()


# ---- 7. the graph ------------------------------------------------------------------------------------------------------------------
def _run_with_graph(graph):
    """N_SCANS scans, then one frame forced in by alego_lm_add_keyframe; the variances alego_regcov_get read right after every archived frame"""
    h = _slam_handle(graph)
    after = {}   # archived frame id -> the record read right after the scan that archived it
    for k in range(N_SCANS):
        n0 = h.map_status()[0]
        h.scan_process(_scan(k), stages=7)
        n1 = h.map_status()[0]
        assert n1 - n0 in (0, 1)
        if n1 > n0:
            after[n0] = h.regcov_get([0])[0]
    kf = h.lm_get_keyframe(-1)
    forced = h.map_status()[0]
    pose = kf["pose"].copy(); pose[0] += 0.5
    h.lm_add_keyframe(pose, kf["corner"], kf["surf"], kf["outlier"])
    assert h.map_status()[0] == forced + 1
    return h, after, forced


@pytest.mark.gpu
def test_odometry_edges_carry_the_registration_variances():
    h, after, forced = _run_with_graph(1)
    try:
        e = h.graph_get_edges(0)
        n = forced + 1
        assert len(e["to"]) == n >= 7 and e["frm"][0] == -1
        assert_bit_equal(e["variance"][0], ODOM_VAR, "the prior")
        assert_bit_equal(e["variance"][forced], ODOM_VAR, "the frame alego_lm_add_keyframe inserted")
        genuine = 0
        for i in range(1, forced):
            rec = after[i]
            if rec["status"] == 1:
                assert_bit_equal(e["variance"][i], rec["variance"], f"edge {i - 1} -> {i}")
                assert not np.array_equal(rec["variance"], ODOM_VAR)
                genuine += 1
            else:
                assert_bit_equal(e["variance"][i], ODOM_VAR, f"edge {i - 1} -> {i} (status {rec['status']})")
        assert genuine >= 5, genuine
        print("variances of the last registered edge (rad^2 x 3, m^2 x 3):", e["variance"][forced - 1])
        # merge, move, thin, optimise, marginals and the gate read `variance` per edge: the device's marginals of this graph against the host twin on
        # the pulled edges, within eps * cond(Lambda) of the block's scale (the bound of tests/test_graph_cov.py)
        kp = np.array([h.map_get_keyframe(j)["pose"] for j in range(n)], F32).reshape(-1, 6)
        X = R.from_pose6(kp)
        g = R.Graph(e["frm"], e["to"], e["between"], e["variance"])
        _, J = g.jacobian(X)
        rel = 2.2e-16 * float(np.linalg.cond((J.T @ J).toarray()))
        assert rel <= 1e-4, rel
        res, cov = h.graph_marginals([0])
        twin, _ = binding.graph_covariance_host(X, e["frm"], e["to"], e["between"], e["variance"])
        assert res[0]["status"] == 1 and res[0]["n_poses"] == n
        frac = max(np.abs(cov[0, k] - twin[k]).max() / (rel * np.abs(twin[k]).max()) for k in range(n))
        print(f"marginals of {n} poses with registration variances: eps*cond {rel:.2e}, device - twin as a fraction of the bound {frac:.4f}")
        assert frac <= 1.0
        # and a candidate edge is judged against them
        chk = h.graph_check_edges([0], [n - 1], [0], [R.between(X[n - 1], X[0])], [np.full(6, 0.1)])
        assert chk[0]["status"] == 1 and chk[0]["d2"] < binding.GRAPH_CHI2_6_999
    finally:
        h.close()


@pytest.mark.gpu
def test_graph_0_leaves_every_edge_alone():
    h, after, forced = _run_with_graph(0)
    try:
        e = h.graph_get_edges(0)
        assert sum(r["status"] == 1 for r in after.values()) >= 5
        for i in range(forced + 1):
            assert_bit_equal(e["variance"][i], ODOM_VAR, f"edge {i}")
    finally:
        h.close()


# ---- 8. a localising handle ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_localising_handle(stream_log):
    hs, _ = stream_log
    nf = hs.map_status()[0]
    frames = [hs.map_get_keyframe(i) for i in range(nf)]
    frames = [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames]
    p = _params()
    h = binding.Handle(p)
    try:
        h.loc_enable(frames, 20.0)
        h.regcov_enable()
        ones = 0
        for k in range(8):
            h.scan_process(_scan(k), stages=7)
            gi, rec = h.debug_get("lm_info"), h.regcov_get([0])[0]
            assert gi[LI_NKF] == 0
            if gi[LI_RUN]:
                assert rec["frame"] == gi[LI_FRAME] and rec["status"] == (1 if gi[LI_OPTIMIZED] else 0), (k, rec["status"])
                ones += rec["status"] == 1
        assert ones >= 3, ones
    finally:
        h.close()
    # off the map: the window is empty, the solver is skipped, the record says so
    h = binding.Handle(p)
    try:
        h.loc_enable(frames, 6.0)
        h.regcov_enable()
        h.lm_apply_correction(np.c_[np.eye(3), [500.0, 500.0, 3.0]])
        ran = 0
        for k in range(6):
            h.scan_process(_scan(k), stages=7)
            gi, rec = h.debug_get("lm_info"), h.regcov_get([0])[0]
            if gi[LI_RUN]:
                assert gi[LI_REC_CNT] == 0 and not gi[LI_OPTIMIZED]
                assert rec["status"] == 0 and rec["frame"] == gi[LI_FRAME] and not any(np.any(rec[key]) for key in REC_FLOATS), (k, rec["status"])
                ran += 1
        assert ran >= 2
    finally:
        h.close()


# ---- the C++ example --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cpp_example_prints_one_record_per_key_frame():
    """examples/replay --regcov / --regcov-graph: one "regcov:" line per key frame, and the run's JSON line is the one of a run without the flag"""
    import json
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "replay")
    runs = {}
    for flag in ((), ("--regcov",), ("--regcov-graph",)):
        r = subprocess.run([exe, "32", *flag], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (flag, r.stderr[-2000:])
        lines = r.stdout.strip().split("\n")
        runs[flag] = (json.loads(lines[-1]), [l.split() for l in lines if l.startswith("regcov:")])
    plain = runs[()][0]
    assert plain["key_frames"] >= 3 and not runs[()][1]
    for flag in (("--regcov",), ("--regcov-graph",)):
        js, recs = runs[flag]
        assert js == plain, flag
        assert len(recs) == js["key_frames"]
        good = [l for l in recs if l[l.index("status") + 1] == "1"]
        assert len(good) >= 2 and recs[0][recs[0].index("status") + 1] == "0", recs   # the first key frame is saved without a map to register against
        for l in good:
            v = [float(x) for x in l[l.index("variance") + 1:]]
            assert len(v) == 6 and all(x > 0 for x in v) and float(l[l.index("eig_min") + 1]) > 0 and int(l[l.index("rows") + 1]) > 100, l
    assert runs[("--regcov",)][1] == runs[("--regcov-graph",)][1]   # (the graph's default odometry variances are the default var_min either way)


# ---- 9. misuse -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misuse():
    p = _params()
    err = lambda: pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_ARG}\)")
    L = binding.lib()
    h = binding.Handle(p, n_slots=2)
    try:
        with err():
            h.regcov_get([0])                                                   # the feature is off
        with err():
            h.regcov_enable(binding.regcov_opts(var_min=[2.0] * 6))             # above the default var_max
        with err():
            h.regcov_enable(binding.regcov_opts(var_min=[0.5] * 6, var_max=[0.1] * 6))
        with err():
            h.regcov_enable(binding.regcov_opts(sigma0=float("nan")))
        with err():
            h.regcov_enable(binding.regcov_opts(graph=1))                       # no graph on this handle
        assert L.alego_regcov_enable(None, None) == binding.ERR_ARG
        h.regcov_enable(binding.regcov_opts(var_min=[0.1] * 6, var_max=[0.1] * 6))   # equal bounds are allowed
        with err():
            h.regcov_enable()                                                   # twice
        recs = h.regcov_get([1, 0])                                             # before any mapping frame
        assert [r["status"] for r in recs] == [0, 0] and all(r["frame"] == 0 and not np.any(r["cov"]) for r in recs)
        for bad in ([2], [-1], [0, 0], [0, 1, 0]):
            with err():
                h.regcov_get(bad)
        out = (binding.RegCov * 2)()
        sl = np.array([0, 1], np.int32)
        assert L.alego_regcov_get(h._h, None, 2, out) == binding.ERR_ARG
        assert L.alego_regcov_get(h._h, sl.ctypes.data, 2, None) == binding.ERR_ARG
        assert L.alego_regcov_get(h._h, sl.ctypes.data, -1, out) == binding.ERR_ARG
        assert L.alego_regcov_get(None, sl.ctypes.data, 2, out) == binding.ERR_ARG
        assert h.regcov_get([]) == []
        one = np.zeros(6)
        assert L.alego_debug_regcov(h._h, None, None, 0, None, 0, out) == binding.ERR_ARG
        assert L.alego_debug_regcov(h._h, one.ctypes.data, None, 3, None, 0, out) == binding.ERR_ARG
        with err():
            h.dist_init(0, 1, binding.dist_unique_id())                         # a sharded registration and the feature exclude each other
    finally:
        h.close()
    h = binding.Handle(p)
    try:
        h.scan_process(_scan(0), stages=7)
        h.scan_process(_scan(1), stages=7)                                      # the first mapping frame
        assert h.debug_get("lm_info")[LI_FRAME] > 0
        with err():
            h.regcov_enable()
    finally:
        h.close()
    h = binding.Handle(p)
    try:
        h.dist_init(0, 1, binding.dist_unique_id())                             # sharded over a communicator of one rank
        with err():
            h.regcov_enable()
        h.dist_shutdown()
    finally:
        h.close()
