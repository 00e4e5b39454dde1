"""-m gpu: lm_solve_remap (kernels_lm.hip) — LaserMapping's registration holding degenerate directions at the prediction,
through alego_remap_enable / alego_remap_get / alego_debug_remap_solve.

The reference is tests/remap_ref.py (numpy.linalg.eigh, the explicitly inverted M, the trust-region loop written out with the projection).
Counts, statuses, iteration and termination words and everything compared between two device runs are exact.

Doubles are asserted at 16 x the largest deviation measured on the MI355X (the project's convention, tests/test_regcov_gpu.py), relative as in
tests/test_remap_math.py — eigenvalues to lambda_max, proj to its largest entry, costs to themselves — parameters and the shift along a held
direction absolute (their caps, 1e-6 and 1e-12 m, are far above):
                                                        eigenvalues  proj      parameters  costs     shift
    kernel on given rows against numpy (DEBUG_CASES)    4.63e-15     5.33e-15  3.77e-14    1.13e-14  5.48e-16
    mapping frames of the synthetic stream              3.17e-15     2.39e-15  1.99e-15    -         -
(The largest parameter and cost figures are those of rows_6: six rows, a problem without a unique minimum, twenty iterations.)"""
import json
import os
import subprocess

import numpy as np
import pytest

import regcov_ref as ref
import remap_ref as rr
from alego_amd import binding
from util import assert_bit_equal, assert_same_record, lm_observables as _observables, reg_params as _params, reg_rows_of_frame as _rows_of_frame, reg_scan as _scan

LI_NKF, LI_RUN, LI_FRAME, LI_FLAGS, LI_NCC, LI_NSC, LI_SUM0, LI_SUM1, LI_OPTIMIZED, LI_NCUR_C, LI_NTOTAL_DS, LI_REC_CNT = 0, 2, 4, 5, 6, 7, 8, 9, 11, 19, 23, 26
LD_PARAMS_IT, LD_COSTS = 27, 39
# 16 x the header's figures
TOL_DEBUG = dict(eigval=7.41e-14, proj=8.53e-14, params=6.03e-13, costs=1.81e-13, shift=8.77e-15)
TOL_STREAM = dict(eigval=5.07e-14, proj=3.82e-14, params=3.18e-14)
REC_FLOATS = ("start", "eigval", "eigvec", "proj")
N_SCANS = 14


def _same_record(a, b, what):
    assert_same_record(a, b, what, ("status", "n_held", "frame"), REC_FLOATS)


def _same_solve(a, b, what):
    for k in ("params_it", "costs", "iterations", "successful", "termination"):
        assert_bit_equal(np.asarray(a[k]), np.asarray(b[k]), f"{what}: {k}")


# ---- 1. the kernel alone on given rows ---------------------------------------------------------------------------------------------
def _debug_cases():
    """name -> (start, edge rows, plane rows, eig_min): the constructed cases and the reduction's edges (LM_SOLVE_T = 256 threads stride over the rows)"""
    c = {k: v[:4] for k, v in rr.CASES.items()}
    for n in (0, 6, 7, 255, 256, 257, 1000):
        p, E, S = ref.courtyard(n_edge=n // 2, n_plane=n - n // 2, seed=400 + n)
        c[f"rows_{n}"] = (p + np.array([0.1, -0.05, 0.04, 0.01, 0.01, -0.01]), E, S, rr.EIG_MIN)
    return c


DEBUG_CASES = _debug_cases()
_WANT = {}


def _want(name, remap, P):
    """the numpy restatement of a case, computed once"""
    if (name, remap) not in _WANT:
        x0, E, S, eig_min = DEBUG_CASES[name]
        _WANT[(name, remap)] = rr.frame(x0, E, S, bool(remap), eig_min, P.huber_delta, P.lm_max_iters, P.lm_outer_iters)
    return _WANT[(name, remap)]


_HANDLES = {}


@pytest.fixture(scope="module")
def debug_handles():
    """one handle per eig_min of the cases (the debug entry takes the handle's option)"""
    def get(eig_min):
        if eig_min not in _HANDLES:
            h = binding.Handle(_params())
            h.remap_enable(binding.remap_opts(eig_min))
            _HANDLES[eig_min] = h
        return _HANDLES[eig_min]
    yield get
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _deviations(got, want, with_rec):
    f = dict(params=np.abs(got["params_it"] - want["params_it"]).max(), costs=0.0)
    nz = want["costs"] != 0
    if nz.any():
        f["costs"] = (np.abs(got["costs"] - want["costs"])[nz] / np.abs(want["costs"][nz])).max()
    if with_rec and want["rec"]["status"] == 1:
        f["eigval"] = np.abs(got["rec"]["eigval"] - want["rec"]["eigval"]).max() / np.abs(want["rec"]["eigval"]).max()
        f["proj"] = np.abs(got["rec"]["proj"] - want["rec"]["proj"]).max() / max(np.abs(want["rec"]["proj"]).max(), 1.0)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEBUG_CASES))
def test_kernel_on_given_rows_against_numpy(debug_handles, name):
    x0, E, S, eig_min = DEBUG_CASES[name]
    h = debug_handles(eig_min)
    P = h.params
    assert P.lm_outer_iters == 2
    got1, got0 = h.debug_remap_solve(x0, E, S, 1), h.debug_remap_solve(x0, E, S, 0)
    want1, want0 = _want(name, 1, P), _want(name, 0, P)
    rec, wrec = got1["rec"], want1["rec"]
    near = wrec["status"] == 1 and np.any(np.abs(wrec["eigval"] - eig_min) <= 1e-3 * eig_min)
    assert not near, (name, wrec["eigval"])   # (a premise of every case: the held count does not hang on rounding)
    f1, f0 = _deviations(got1, want1, True), _deviations(got0, want0, False)
    shift = np.abs(rr.held_shift(dict(wrec, start=x0), got1["params_it"][1])).max() if wrec["n_held"] else 0.0
    print(f"{name}: status {rec['status']} held {rec['n_held']} iterations {got1['iterations']} / plain {got0['iterations']} termination {got1['termination']} / {got0['termination']}; "
          "device - numpy, remap " + "  ".join(f"{k} {v:.2e}" for k, v in f1.items()) + "; plain " + "  ".join(f"{k} {v:.2e}" for k, v in f0.items()) + f"; shift {shift:.2e}")
    # exact: the record's integers, the start, the iteration and termination words
    assert (rec["status"], rec["n_held"], rec["frame"]) == (wrec["status"], wrec["n_held"], 0), (name, rec["status"], rec["n_held"])
    assert np.array_equal(rec["start"], x0)
    assert rec["status"] == (1 if len(E) + len(S) > 6 else 0)
    for got, want, tag in ((got1, want1, "remap"), (got0, want0, "plain")):
        for k in ("iterations", "successful", "termination"):
            assert list(got[k]) == list(want[k]), (name, tag, k, got[k], want[k])
    if rec["status"] != 1:
        assert not any(np.any(rec[k]) for k in ("eigval", "eigvec", "proj"))
    for k, v in f1.items():
        assert v <= TOL_DEBUG[k], (name, "remap", k, v, TOL_DEBUG[k])
    for k, v in f0.items():
        assert v <= TOL_DEBUG[k], (name, "plain", k, v, TOL_DEBUG[k])
    assert shift <= TOL_DEBUG["shift"], (name, shift)
    if name in rr.SPURIOUS:   # the premise on the device: the plain kernel is dragged along the corridor
        moved = rr.held_shift(dict(wrec, start=x0), got0["params_it"][1])
        assert abs(moved[0]) > 0.1, (name, moved)
    if rec["n_held"] == 0:
        _same_solve(got1, got0, f"{name}: nothing held, lm_solve_remap against lm_solve")
        if rec["status"] == 1:
            assert np.array_equal(rec["proj"], np.eye(6))
    if rec["n_held"] == 6:
        assert not np.any(rec["proj"]) and list(got1["termination"]) == [2, 2]
        assert_bit_equal(got1["params_it"], np.tile(x0, (2, 1)), f"{name}: everything held")


@pytest.mark.gpu
def test_full_eval_twins_are_bit_equal(debug_handles):
    for name in ("spurious_3_0.5", "courtyard_100", "courtyard_1e5", "rows_257", "rows_1000", "rows_7"):
        x0, E, S, eig_min = DEBUG_CASES[name]
        h = debug_handles(eig_min)
        base = [h.debug_remap_solve(x0, E, S, r) for r in (0, 1)]
        h.set_option("ALEGO_SOLVE_FULL_EVAL", 1)
        try:
            full = [h.debug_remap_solve(x0, E, S, r) for r in (0, 1)]
        finally:
            h.set_option("ALEGO_SOLVE_FULL_EVAL", 0)
        for r in (0, 1):
            _same_solve(full[r], base[r], f"{name} remap {r}: _full_eval against the default kernel")
        _same_record(full[1]["rec"], base[1]["rec"], name)


@pytest.mark.gpu
def test_kernel_statuses(debug_handles):
    h = debug_handles(rr.EIG_MIN)
    x0, E, S, _ = DEBUG_CASES["rows_257"]
    up = x0.copy(); up[4] = np.pi / 2
    r = h.debug_remap_solve(up, E, S, 1)["rec"]
    assert r["status"] == -3 and r["n_held"] == 0 and not np.any(r["proj"]) and np.array_equal(r["start"], up)
    bad = E.copy(); bad[5, 0] = np.nan
    r = h.debug_remap_solve(x0, bad, S, 1)
    assert r["rec"]["status"] == -2 and r["rec"]["n_held"] == 0 and not np.any(r["rec"]["eigvec"])
    _same_solve(r, h.debug_remap_solve(x0, bad, S, 0), "a status other than 1 holds nothing")


# ---- 2. mapping frames of the synthetic stream ---------------------------------------------------------------------------------------
def _run_stream(h, n=N_SCANS, regcov=False):
    log = []
    for k in range(n):
        flags, odom, mp = h.scan_process(_scan(k), stages=7)
        gi, E, S = _rows_of_frame(h)
        st = h.debug_get("lm_state")
        log.append(dict(k=k, gi=gi, E=E, S=S, rec=h.remap_get([0])[0], params_it=st[LD_PARAMS_IT:LD_PARAMS_IT + 12].reshape(2, 6).copy(),
                        rc=h.regcov_get([0])[0] if regcov else None))
    return log


@pytest.fixture(scope="module")
def stream_log():
    h = binding.Handle(_params())
    h.map_enable(64, 1 << 19)
    h.remap_enable(binding.remap_opts(rr.EIG_MIN))
    log = _run_stream(h)
    yield h, log
    h.close()


@pytest.mark.gpu
def test_mapping_frames_against_numpy(stream_log):
    h, log = stream_log
    P = h.params
    seen = held = left_out = 0
    worst = {k: 0.0 for k in TOL_STREAM}
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
            assert gi[LI_FLAGS] & 16 and rec["status"] == 0 and rec["n_held"] == 0 and not np.any(rec["proj"]), (e["k"], rec["status"])
            continue
        assert (gi[LI_NCC], gi[LI_NSC]) == (len(e["E"]), len(e["S"])), e["k"]
        want = rr.frame(rec["start"], e["E"], e["S"], True, rr.EIG_MIN, P.huber_delta, P.lm_max_iters, P.lm_outer_iters)
        wrec = want["rec"]
        if np.any(np.abs(wrec["eigval"] - rr.EIG_MIN) <= 1e-3 * rr.EIG_MIN):
            left_out += 1
            continue
        assert rec["status"] == wrec["status"] == 1 and rec["n_held"] == wrec["n_held"], (e["k"], rec["n_held"], wrec["n_held"], wrec["eigval"])
        f = dict(eigval=np.abs(rec["eigval"] - wrec["eigval"]).max() / wrec["eigval"][-1], proj=np.abs(rec["proj"] - wrec["proj"]).max() / max(np.abs(wrec["proj"]).max(), 1.0),
                 params=np.abs(e["params_it"] - want["params_it"]).max())
        summ = [int(gi[LI_SUM0]), int(gi[LI_SUM1])]
        print(f"scan {e['k']}: {len(e['E'])} edges {len(e['S'])} planes, eigenvalues {rec['eigval'][0]:.3g} {rec['eigval'][1]:.3g} .. {rec['eigval'][5]:.3g}, held {rec['n_held']}, "
              f"iterations {[s & 255 for s in summ]} termination {[s >> 16 for s in summ]}; device - numpy " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
        assert [s & 255 for s in summ] == list(want["iterations"]) and [s >> 16 for s in summ] == list(want["termination"]), (e["k"], summ, want["iterations"], want["termination"])
        worst = {k: max(worst[k], f[k]) for k in f}
        seen += 1
        held += rec["n_held"] >= 1
    print("largest over the frames: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()), f"; {seen} frames, {held} with a held direction, {left_out} left out")
    assert seen >= 5 and held >= 1 and left_out <= 1, (seen, held, left_out)
    for k, v in worst.items():
        assert v <= TOL_STREAM[k], (k, v, TOL_STREAM[k])


# ---- 3. nothing else moves -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_else_moves_when_nothing_is_held():
    p = _params()
    A, B = binding.Handle(p, n_slots=2), binding.Handle(p, n_slots=2)
    try:
        B.remap_enable(binding.remap_opts(1e-300))
        for k in range(N_SCANS):
            for s in (0, 1):
                ra, rb = A.scan_process(_scan(k, s), stages=7, slot=s), B.scan_process(_scan(k, s), stages=7, slot=s)
                assert ra[0] == rb[0], (k, s, ra[0], rb[0])
                for i in (1, 2):
                    for key in ("t", "q", "params"):
                        assert_bit_equal(ra[i][key], rb[i][key], f"scan {k} slot {s}: pose {i} {key}")
            if k % 4 == 3 or k == N_SCANS - 1:
                for s in (0, 1):
                    oa, ob = _observables(A, s), _observables(B, s)
                    for key in oa:
                        assert_bit_equal(oa[key], ob[key], f"scan {k} slot {s}: {key}")
        for s in (0, 1):
            assert A.lm_keyframe_count(s) == B.lm_keyframe_count(s) >= 5
            ka, kb = A.lm_get_keyframe(-1, slot=s), B.lm_get_keyframe(-1, slot=s)
            for key in ("pose", "corner", "surf", "outlier"):
                assert_bit_equal(ka[key], kb[key], f"slot {s}: newest key frame {key}")
        recs = B.remap_get([0, 1])
        assert all(r["status"] == 1 and r["n_held"] == 0 and np.array_equal(r["proj"], np.eye(6)) for r in recs)
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_a_slot_does_not_depend_on_its_company():
    p = _params()
    H3 = binding.Handle(p, n_slots=3)
    singles = [binding.Handle(p) for _ in range(3)]
    try:
        for h in [H3] + singles:
            h.remap_enable()
        held = 0
        for k in range(10):
            for s in range(3):
                H3.scan_process(_scan(k, s), stages=7, slot=s)
                singles[s].scan_process(_scan(k, s), stages=7)
            got = H3.remap_get([2, 0, 1])
            for s, g in zip((2, 0, 1), got):
                _same_record(g, singles[s].remap_get([0])[0], f"scan {k} slot {s}")
                assert_bit_equal(H3.debug_get("lm_state", slot=s), singles[s].debug_get("lm_state"), f"scan {k} slot {s}: lm_state")
                held += g["n_held"] >= 1
        assert held >= 1
    finally:
        H3.close()
        for h in singles:
            h.close()


# ---- 4. everything held ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_everything_held_keeps_the_prediction():
    h = binding.Handle(_params())
    try:
        h.remap_enable(binding.remap_opts(1e30))
        seen = 0
        for e in _run_stream(h, 10):
            gi, rec = e["gi"], e["rec"]
            if not (gi[LI_RUN] and gi[LI_OPTIMIZED]):
                continue
            assert rec["status"] == 1 and rec["n_held"] == 6 and not np.any(rec["proj"]), (e["k"], rec["n_held"])
            assert_bit_equal(e["params_it"], np.tile(rec["start"], (2, 1)), f"scan {e['k']}: params_ after both solves")
            assert (gi[LI_SUM0] >> 16, gi[LI_SUM1] >> 16) == (2, 2), (e["k"], gi[LI_SUM0], gi[LI_SUM1])
            seen += 1
        assert seen >= 3, seen
    finally:
        h.close()


# ---- 5. with the registration covariance on as well ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_regcov_on_as_well(stream_log):
    _, plain = stream_log
    h = binding.Handle(_params())
    try:
        h.map_enable(64, 1 << 19)
        h.regcov_enable()
        h.remap_enable(binding.remap_opts(rr.EIG_MIN))
        ones = 0
        for e, e0 in zip(_run_stream(h, N_SCANS, regcov=True), plain):
            gi, rec, rc = e["gi"], e["rec"], e["rc"]
            _same_record(rec, e0["rec"], f"scan {e['k']}: the record does not depend on alego_regcov_enable")
            assert_bit_equal(e["params_it"], e0["params_it"], f"scan {e['k']}: params_")
            if gi[LI_RUN] and gi[LI_OPTIMIZED]:
                assert rc["status"] == 1 and rc["frame"] == gi[LI_FRAME] == rec["frame"], (e["k"], rc["status"])
                assert rc["n_degenerate"] == int((rc["eigval"] < rr.EIG_MIN).sum())
                if rec["n_held"] >= 1 and rc["eigval"][0] < rr.EIG_MIN:
                    assert rc["n_degenerate"] >= 1
                ones += 1
        assert ones >= 5
    finally:
        h.close()


# ---- 6. a localising handle ------------------------------------------------------------------------------------------------------------
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
        h.remap_enable()
        ones = 0
        for k in range(8):
            h.scan_process(_scan(k), stages=7)
            gi, rec = h.debug_get("lm_info"), h.remap_get([0])[0]
            assert gi[LI_NKF] == 0
            if gi[LI_RUN]:
                assert rec["frame"] == gi[LI_FRAME] and rec["status"] == (1 if gi[LI_OPTIMIZED] else 0), (k, rec["status"])
                ones += rec["status"] == 1
        assert ones >= 3, ones
    finally:
        h.close()
    h = binding.Handle(p)   # off the map: the window is empty, the solver is skipped, the record says so
    try:
        h.loc_enable(frames, 6.0)
        h.remap_enable()
        h.lm_apply_correction(np.c_[np.eye(3), [500.0, 500.0, 3.0]])
        ran = 0
        for k in range(6):
            h.scan_process(_scan(k), stages=7)
            gi, rec = h.debug_get("lm_info"), h.remap_get([0])[0]
            if gi[LI_RUN]:
                assert gi[LI_REC_CNT] == 0 and not gi[LI_OPTIMIZED]
                assert rec["status"] == 0 and rec["frame"] == gi[LI_FRAME] and rec["n_held"] == 0 and not any(np.any(rec[key]) for key in ("eigval", "eigvec", "proj")), (k, rec["status"])
                ran += 1
        assert ran >= 2
    finally:
        h.close()


# ---- 7. misuse, and the C++ example ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misuse():
    p = _params()
    err = lambda: pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_ARG}\)")
    L = binding.lib()
    h = binding.Handle(p, n_slots=2)
    try:
        with err():
            h.remap_get([0])                                                    # the feature is off
        for v in (float("nan"), float("inf")):
            with err():
                h.remap_enable(binding.remap_opts(v))
        assert L.alego_remap_enable(None, None) == binding.ERR_ARG
        h.remap_enable(binding.remap_opts(-1.0))                                # <= 0: the default
        with err():
            h.remap_enable()                                                    # twice
        recs = h.remap_get([1, 0])                                              # before any mapping frame
        assert [r["status"] for r in recs] == [0, 0] and all(r["frame"] == 0 and not np.any(r["proj"]) for r in recs)
        for bad in ([2], [-1], [0, 0], [0, 1, 0]):
            with err():
                h.remap_get(bad)
        out = (binding.Remap * 2)()
        sl = np.array([0, 1], np.int32)
        assert L.alego_remap_get(h._h, None, 2, out) == binding.ERR_ARG
        assert L.alego_remap_get(h._h, sl.ctypes.data, 2, None) == binding.ERR_ARG
        assert L.alego_remap_get(h._h, sl.ctypes.data, -1, out) == binding.ERR_ARG
        assert L.alego_remap_get(None, sl.ctypes.data, 2, out) == binding.ERR_ARG
        assert h.remap_get([]) == []
        one, pit, costs, summ = np.zeros(6), np.zeros(12), np.zeros(4), np.zeros(2, np.int32)
        assert L.alego_debug_remap_solve(h._h, None, None, 0, None, 0, 1, pit.ctypes.data, costs.ctypes.data, summ.ctypes.data, None) == binding.ERR_ARG
        assert L.alego_debug_remap_solve(h._h, one.ctypes.data, None, 3, None, 0, 1, pit.ctypes.data, costs.ctypes.data, summ.ctypes.data, None) == binding.ERR_ARG
        assert L.alego_debug_remap_solve(h._h, one.ctypes.data, None, 0, None, 0, 1, None, costs.ctypes.data, summ.ctypes.data, None) == binding.ERR_ARG
        assert L.alego_debug_remap_solve(h._h, one.ctypes.data, None, 0, None, 0, 1, pit.ctypes.data, costs.ctypes.data, summ.ctypes.data, None) == 0
        with err():
            h.dist_init(0, 1, binding.dist_unique_id())                         # a sharded registration and the mode exclude each other
    finally:
        h.close()
    h = binding.Handle(p)
    try:
        h.scan_process(_scan(0), stages=7)
        h.scan_process(_scan(1), stages=7)                                      # the first mapping frame
        assert h.debug_get("lm_info")[LI_FRAME] > 0
        with err():
            h.remap_enable()
    finally:
        h.close()
    h = binding.Handle(p)
    try:
        h.dist_init(0, 1, binding.dist_unique_id())                             # sharded over a communicator of one rank
        with err():
            h.remap_enable()
        h.dist_shutdown()
    finally:
        h.close()


@pytest.mark.gpu
def test_cpp_example_prints_one_line_per_key_frame():
    """examples/replay --remap [EIG_MIN]: one "remap:" line per key frame (n_held, the smallest eigenvalue), exit code 0"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "replay")
    r = subprocess.run([exe, "40", "--remap"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    js = json.loads(lines[-1])
    recs = [l.split() for l in lines if l.startswith("remap:")]
    assert js["key_frames"] >= 3 and len(recs) == js["key_frames"], (js, len(recs))
    good = [l for l in recs if l[l.index("status") + 1] == "1"]
    assert len(good) >= 2
    for l in good:
        assert 0 <= int(l[l.index("n_held") + 1]) <= 6 and float(l[l.index("eig_min") + 1]) > -1e-6
    # an eig_min nothing falls below: the same lines with nothing held, and the run's JSON line is the one of a run without the flag
    r0 = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=120)
    r2 = subprocess.run([exe, "40", "--remap", "1e-300"], capture_output=True, text=True, timeout=120)
    assert r0.returncode == 0 and r2.returncode == 0
    assert not [l for l in r0.stdout.split("\n") if l.startswith("remap:")]
    none_held = [l.split() for l in r2.stdout.split("\n") if l.startswith("remap:")]
    assert json.loads(r2.stdout.strip().split("\n")[-1]) == json.loads(r0.stdout.strip().split("\n")[-1])
    assert len(none_held) == json.loads(r2.stdout.strip().split("\n")[-1])["key_frames"] and all(l[l.index("n_held") + 1] == "0" for l in none_held)
