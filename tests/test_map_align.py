"""Aligning one slot's key-frame archive to another's by appearance (alego_map_align, kernels_reloc.hip / align_math.h):
several source frames are searched in the destination's descriptors, verified by the ICP of alego_loop_search, and the hypotheses decide
among themselves which rigid transform takes the source archive into the destination's frame.

References: numpy restatements of the query rule, of the agreement test and of the consensus (the f64 arithmetic written out in the order
csrc/align_math.h uses), the numpy descriptor and match of tests/test_relocalize.py, and the UNCHANGED oracle's loop_icp through
tests/test_loop_appearance.py::emulate — the source frame is handed to it as frame nd of an archive one longer than the destination's, so
that its window is the destination's [i - lc_search_num, i + lc_search_num] within [0, nd - 1].

The synthetic world repeats under a half turn: a source frame whose true place is outside the destination stretch
but whose mirror place is inside it yields an aliased hypothesis that the ICP accepts.  The two lap cases below are chosen on the CPU so
that the emulation alone decides correctly; the tables they print are quoted in DESIGN.md section 17, and A / B there come from
measure_tolerances().
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from test_loop_appearance import MAX_RANGE, Z_OFFSET, _sparse, add_frames, cloud_of, emulate, la_desc, split3, world_correction_np
from test_loop_search import LAP, _initial_guess, _params, device_ref, oracle_replay, replay_handle
from test_relocalize import ANG_TOL, POS_TOL, desc_np, guess_of, match_all_np
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["alego_map_align", "alego_map_align_queries", "alego_map_align_consensus", "alego_map_align_poses"]
MAXQ = binding.ALIGN_MAX_QUERIES
TOL_T, TOL_R = binding.ALIGN_TOL_TRANS, binding.ALIGN_TOL_ROT
EMPTY = np.zeros((0, 4), F32)
# the two lap cases: (name, destination (first scan, scans), source (first scan, scans)); chosen with the emulation
LAP_CASES = [("no mirror overlap", (0, 251), (100, 171)), ("a minority of aliased hypotheses", (0, 251), (100, 431))]


def _O():
    from oracle import oracle_py
    return oracle_py


# ---- the rule in numpy ----------------------------------------------------------------------------------------------------------
def queries_np(ns, n_queries):
    Q = min(n_queries, max(ns, 0))
    return np.array([((2 * q + 1) * ns) // (2 * Q) for q in range(Q)], np.int32)


def disagreement_np(Ta, pa, Tb, pb):
    """(rad, m at p_a, m at p_b) of two hypotheses: csrc/align_math.h's arithmetic, f64, every sum in its order"""
    A = [[float(v) for v in r] for r in np.asarray(Ta, F32).reshape(4, 4)]
    B = [[float(v) for v in r] for r in np.asarray(Tb, F32).reshape(4, 4)]
    with np.errstate(all="ignore"):
        M = [[np.float64(A[0][i]) * B[0][j] + np.float64(A[1][i]) * B[1][j] + np.float64(A[2][i]) * B[2][j] for j in range(3)] for i in range(3)]
        c = 0.5 * (((M[0][0] + M[1][1]) + M[2][2]) - 1.0)
        v = [0.5 * (M[2][1] - M[1][2]), 0.5 * (M[0][2] - M[2][0]), 0.5 * (M[1][0] - M[0][1])]
        s = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) if np.isfinite(v).all() else float("nan")
        ang = math.atan2(s, c)
        out = [ang]
        for p in (pa, pb):
            p = [float(x) for x in np.asarray(p, F32).reshape(3)]
            d = []
            for r in range(3):
                ya = ((np.float64(A[r][0]) * p[0] + np.float64(A[r][1]) * p[1]) + np.float64(A[r][2]) * p[2]) + A[r][3]
                yb = ((np.float64(B[r][0]) * p[0] + np.float64(B[r][1]) * p[1]) + np.float64(B[r][2]) * p[2]) + B[r][3]
                d.append(ya - yb)
            q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            out.append(math.sqrt(q) if q >= 0 else float("nan"))
    return tuple(float(x) for x in out)


def agree_np(Ta, pa, Tb, pb, tol_t, tol_r):
    ang, da, db = disagreement_np(Ta, pa, Tb, pb)
    return bool(ang <= tol_r and da <= tol_t and db <= tol_t)


def consensus_np(T, pos, fitness, accepted, tol_t, tol_r):
    """(support (n,), best): the largest support (>= 1), ties to the smaller fitness, then to the smaller index"""
    n = len(T)
    sup = np.zeros(n, np.int32)
    for a in range(n):
        sup[a] = sum(1 for b in range(n) if accepted[a] and accepted[b] and agree_np(T[a], pos[a], T[b], pos[b], tol_t, tol_r))
    best = -1
    for a in range(n):
        if sup[a] >= 1 and (best < 0 or sup[a] > sup[best] or (sup[a] == sup[best] and fitness[a] < fitness[best])):
            best = a
    return sup, best


def rigid(rpy, t):
    T = np.eye(4)
    T[:3, :3] = _initial_guess(np.r_[0, 0, 0, rpy].astype(F32)).astype(np.float64)[:3, :3]
    T[:3, 3] = t
    return T


def inv(T):
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def full(T):
    T = np.asarray(T, np.float64)
    return T if T.shape == (4, 4) else np.vstack([T.reshape(3, 4), [0, 0, 0, 1]])


def gap(Ta, Tb):
    """(m, rad) between two rigid transforms"""
    Ta, Tb = full(Ta), full(Tb)
    M = Ta[:3, :3].T @ Tb[:3, :3]
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])), float(np.arctan2(np.linalg.norm(v), (np.trace(M) - 1.0) / 2.0))   # (arccos loses small angles)


def truth(dst_start, src_start):
    """dst <- src of two archives that each sit in the frame of their first scan: synth.pose(a)^-1 synth.pose(b)"""
    def M(k):
        x, y, z, yaw = synth.pose(k % LAP)
        return rigid([0, 0, yaw], [x, y, z])
    return inv(M(dst_start)) @ M(src_start)


def candidates_np(desc_dst, q, n_cand, max_dist=0):
    """(ids, dists, shifts) of query descriptor q over ALL destination frames: the brute force in (D, id)"""
    none = (np.zeros(0, np.int32),) * 3
    if len(desc_dst) == 0 or not np.asarray(q).any():
        return none
    d, s = match_all_np(desc_dst, q)
    order = np.lexsort((np.arange(len(d)), d))[:n_cand]
    if max_dist > 0:
        keep = np.nonzero(d[order] > max_dist)[0]
        order = order[:keep[0]] if len(keep) else order
    return order.astype(np.int32), d[order].astype(np.int32), s[order].astype(np.int32)


def emulate_pair(p, src, dst, n_queries=8, n_cand=2, max_dist=0, fitness_max=None, tol_t=TOL_T, tol_r=TOL_R, min_support=2):
    """alego_map_align's rule on the reference side.  src / dst: dict(poses (n, 6) f32, frame(j) -> (corner, surf, outlier)).  Returns dict(status,
    best, support, T (4, 4) f64 or None, hyp: per query dict(src_frame, cand (ids, dists, shifts), tried, accepted, dst_frame, shift, dist, want, guess6, T, pos))"""
    ns, nd = len(src["poses"]), len(dst["poses"])
    fmax = p.lc_fitness_max if fitness_max is None else fitness_max
    dd = dst.setdefault("desc", np.array([desc_np(np.concatenate(dst["frame"](j)), MAX_RANGE, Z_OFFSET)[0] for j in range(nd)]).reshape(-1, 60, 20))
    hyp = []
    kp1 = np.concatenate([np.asarray(dst["poses"], F32).reshape(-1, 6), np.zeros((1, 6), F32)])   # (emulate: the source is frame nd of an archive of nd + 1)
    for f in queries_np(ns, n_queries) if nd else []:
        f = int(f)
        sf = tuple(src["frame"](f))
        ids, dists, shifts = candidates_np(dd, desc_np(np.concatenate(sf), MAX_RANGE, Z_OFFSET)[0], n_cand, max_dist)
        h = dict(src_frame=f, cand=(ids, dists, shifts), tried=0, accepted=0, dst_frame=int(ids[0]) if len(ids) else -1, dist=int(dists[0]) if len(ids) else 0,
                 shift=int(shifts[0]) if len(ids) else 0, want=None, guess6=None, T=np.zeros((4, 4)), pos=np.asarray(src["poses"][f][:3], F32), fitness=0.0)
        for k in range(len(ids)):
            i, s = int(ids[k]), int(shifts[k])
            want, g, t_correct, _ = emulate(p, kp1, lambda j: sf if j == nd else dst["frame"](j), i, s)
            h.update(tried=k + 1, dst_frame=i, dist=int(dists[k]), shift=s, want=want, guess6=g, T=world_correction_np(t_correct, src["poses"][f]), fitness=float(want["fitness"]))
            if want["converged"] and want["fitness"] <= fmax:
                h["accepted"] = 1
                break
        hyp.append(h)
    out = dict(hyp=hyp, status=0, best=-1, support=0, T=None, sup=np.zeros(len(hyp), np.int32))
    if any(h["tried"] for h in hyp):
        sup, best = consensus_np([h["T"] for h in hyp], [h["pos"] for h in hyp], [h["fitness"] for h in hyp], [h["accepted"] for h in hyp], tol_t, tol_r)
        out.update(sup=sup, best=best, support=int(sup[best]) if best >= 0 else 0, T=hyp[best]["T"] if best >= 0 else None)
        out["status"] = 2 if best >= 0 and sup[best] >= min_support else 1
    return out


def oracle_stretch(p, start, steps):
    """the oracle's archive of `steps` scans from `start`: dict(poses, frame)"""
    ref = oracle_replay(p, start, steps)
    o, kp = ref["o"], ref["poses"].astype(F32)
    frames = [o.lm_keyframe(i) for i in range(len(kp))]
    o.close()
    return dict(poses=kp, frame=lambda j: frames[j], stamps=ref["stamps"])


def table(em, T_true, tag):
    """the printed table of hypotheses (DESIGN.md section 17 quotes it); returns per hypothesis (m, rad) from the ground truth, NaN where none"""
    err = []
    print(f"{tag}: status {em['status']} best {em['best']} support {em['support']}")
    for q, h in enumerate(em["hyp"]):
        dp, da = gap(h["T"], T_true) if h["tried"] else (float("nan"),) * 2
        err.append((dp, da))
        print(f"  q{q}: src {h['src_frame']:3d} -> dst {h['dst_frame']:3d} D {h['dist']:5d} shift {h['shift']:2d} tried {h['tried']} accepted {h['accepted']} fitness {h['fitness']:.4f} "
              f"support {em['sup'][q]}; {dp:8.3f} m {da:7.4f} rad from the truth")
    return np.array(err).reshape(-1, 2)


def measure_tolerances(cases):
    """A = the largest pairwise disagreement (m, rad) among accepted hypotheses within POS_TOL / ANG_TOL of the ground truth, B = the smallest between
    such a hypothesis and an accepted one that is not; over [(emulation, T_true)]"""
    A, B = [0.0, 0.0], [float("inf"), float("inf")]
    for em, T_true in cases:
        hs = [h for h in em["hyp"] if h["accepted"]]
        ok = [gap(h["T"], T_true)[0] < POS_TOL and gap(h["T"], T_true)[1] < ANG_TOL for h in hs]
        for a in range(len(hs)):
            for b in range(len(hs)):
                if a == b or not ok[a]:
                    continue
                ang, da, db = disagreement_np(hs[a]["T"].astype(F32), hs[a]["pos"], hs[b]["T"].astype(F32), hs[b]["pos"])
                if ok[b]:
                    A = [max(A[0], da, db), max(A[1], ang)]
                else:
                    # two hypotheses disagree when EITHER measure exceeds its tolerance: the margin is in whichever is relatively larger
                    B = [min(B[0], max(da, db)), min(B[1], ang)]
    return A, B


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_map_align_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s
    for t in ("alego_map_align_opts", "alego_map_align_hyp", "alego_map_align_result", "ALEGO_ALIGN_MAX_QUERIES"):
        assert t in hdr, t
    assert float(re.search(r"#define ALEGO_ALIGN_TOL_TRANS (\S+)", hdr).group(1)) == TOL_T and float(re.search(r"#define ALEGO_ALIGN_TOL_ROT (\S+)", hdr).group(1)) == TOL_R


@pytest.mark.parametrize("Q", [1, 8, 32])
def test_queries_twin_equals_numpy(Q):
    for ns in (0, 1, 2, Q - 1, Q, Q + 1, 1000):
        got, want = binding.map_align_queries(ns, Q), queries_np(ns, Q)
        assert np.array_equal(got, want), (ns, Q, got, want)
        assert len(got) == min(Q, ns) and (np.diff(got) > 0).all() and ((got >= 0) & (got < ns)).all(), (ns, Q, got)
    assert np.array_equal(binding.map_align_queries(1000, 0), queries_np(1000, 8)), "n_queries <= 0: 8"
    fr = np.zeros(64, np.int32)
    assert binding.lib().alego_map_align_queries(10, 33, fr.ctypes.data) == binding.ERR_ARG
    assert binding.lib().alego_map_align_queries(-1, 8, fr.ctypes.data) == binding.ERR_ARG


def _hyp(rpy, t):
    return rigid(rpy, t).astype(F32)


def consensus_cases():
    """(name, T (n, 4, 4) f32, pos (n, 3), fitness, accepted, tol_t, tol_r)"""
    rng = np.random.default_rng(5)
    out = []
    z3 = lambda n: np.zeros((n, 3), F32)
    out.append(("n = 0", np.zeros((0, 4, 4), F32), z3(0), [], [], 0.25, 0.02))
    four = np.array([_hyp([0, 0, 0.4], [1, 2, 3]), _hyp([0, 0, 0.401], [1.01, 2, 3]), _hyp([0, 0, 0.4], [40, 2, 3]), _hyp([0.001, 0, 0.4], [40, 2.02, 3])])
    out.append(("none accepted", four, z3(4), [0.1, 0.2, 0.3, 0.4], [0, 0, 0, 0], 0.25, 0.02))
    out.append(("one accepted", four, z3(4), [0.1, 0.2, 0.3, 0.4], [0, 0, 1, 0], 0.25, 0.02))
    out.append(("two disjoint agreeing pairs: the fitness breaks the tie", four, z3(4), [0.3, 0.2, 0.15, 0.4], [1, 1, 1, 1], 0.25, 0.02))
    out.append(("two disjoint agreeing pairs: then the index", four, z3(4), [0.2, 0.2, 0.2, 0.2], [1, 1, 1, 1], 0.25, 0.02))
    base = rigid([0.02, -0.01, 1.1], [12, -7, 0.5])
    allq = np.array([(base @ rigid(rng.uniform(-2e-3, 2e-3, 3), rng.uniform(-0.02, 0.02, 3))).astype(F32) for _ in range(32)])
    out.append(("32 hypotheses that all agree", allq, rng.uniform(-20, 20, (32, 3)).astype(F32), rng.uniform(0.1, 0.2, 32), np.ones(32, np.int32), 0.25, 0.02))
    # a disagreement at the tolerance from below and from above by one f64 step: the side comes from numpy's own evaluation
    Ta, Tb = _hyp([0, 0, 0.25], [3, 4, 5]), _hyp([0, 0, 0.25], [3.125, 4, 5])
    p = np.array([[1.5, -2.5, 0.25]] * 2, F32)
    ang, da, db = disagreement_np(Ta, p[0], Tb, p[1])
    assert da == db and da > 0
    for tt in (np.nextafter(da, 0.0), da, np.nextafter(da, 1.0)):
        out.append((f"translation at the tolerance ({float(tt).hex()})", np.array([Ta, Tb]), p, [0.1, 0.2], [1, 1], float(tt), 0.02))
    Tc = _hyp([0, 0, 0.26], [3, 4, 5])
    ang, da, db = disagreement_np(Ta, z3(1)[0], Tc, z3(1)[0])
    assert ang > 0 and da == 0
    for tr in (np.nextafter(ang, 0.0), ang, np.nextafter(ang, 1.0)):
        out.append((f"rotation at the tolerance ({float(tr).hex()})", np.array([Ta, Tc]), z3(2), [0.1, 0.2], [1, 1], 0.25, float(tr)))
    Td = _hyp([0, 0, 0.253], [3, 4, 5])
    out.append(("a small rotation about the origin, seen from 100 m", np.array([Ta, Td]), np.array([[100, 0, 0], [0, -100, 0]], F32), [0.1, 0.2], [1, 1], 0.25, 0.02))
    out.append(("the same rotation seen from the origin", np.array([Ta, Td]), z3(2), [0.1, 0.2], [1, 1], 0.25, 0.02))
    nf = four.copy()
    nf[0, 1, 3] = np.nan
    nf[3, 0, 0] = np.inf
    out.append(("a non-finite T agrees with nothing", nf, z3(4), [0.1, 0.2, 0.3, 0.4], [1, 1, 1, 1], 0.25, 0.02))
    return out


@pytest.mark.parametrize("case", range(len(consensus_cases())))
def test_consensus_twin_equals_numpy(case):
    name, T, pos, fit, acc, tt, tr = consensus_cases()[case]
    sup, best = binding.map_align_consensus(T, pos, fit, acc, tt, tr)
    wsup, wbest = consensus_np(T, pos, fit, acc, tt, tr)
    assert np.array_equal(sup, wsup) and best == wbest, (name, sup, wsup, best, wbest)
    if name in ("n = 0", "none accepted"):
        assert best == -1 and not sup.any()
    if name == "one accepted":
        assert best == 2 and sup.tolist() == [0, 0, 1, 0]
    if name.startswith("two disjoint"):
        assert sup.tolist() == [2, 2, 2, 2] and best == (2 if "fitness" in name else 0)
    if name.startswith("32"):
        assert (sup == 32).all() and best == int(np.argmin(fit))
    if " at the tolerance" in name:
        d = disagreement_np(T[0], pos[0], T[1], pos[1])
        inside = d[1] <= tt and d[0] <= tr
        assert sup.tolist() == ([2, 2] if inside else [1, 1]), (name, d, sup)
    if name.startswith("a small rotation"):
        assert sup.tolist() == [1, 1], "0.003 rad at 100 m is 0.3 m"
    if name.startswith("the same rotation"):
        assert sup.tolist() == [2, 2]
    if name.startswith("a non-finite"):
        assert sup.tolist() == [0, 1, 1, 0] and best == 1


def test_consensus_tolerance_cases_cover_both_sides():
    sides = {}
    for name, T, pos, fit, acc, tt, tr in consensus_cases():
        if " at the tolerance" in name:
            sides.setdefault(name.split()[0], []).append(binding.map_align_consensus(T, pos, fit, acc, tt, tr)[0].tolist())
    assert sides["translation"] == [[1, 1], [2, 2], [2, 2]] and sides["rotation"] == [[1, 1], [2, 2], [2, 2]], sides


def pose6_of_np(X):
    X = np.asarray(X, np.float64)
    return np.array([X[0, 3], X[1, 3], X[2, 3], math.atan2(X[2, 1], X[2, 2]), math.atan2(-X[2, 0], math.sqrt(X[2, 1] * X[2, 1] + X[2, 2] * X[2, 2])),
                     math.atan2(X[1, 0], X[0, 0])]).astype(F32)


def rzryrx_np(kp):
    """Pose3(Rot3::RzRyRx(roll, pitch, yaw), xyz) of an f32 key pose, f64"""
    x, y, z, r, p, w = (float(v) for v in np.asarray(kp, F32))
    cx, sx, cy, sy, cz, sz = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(w), math.sin(w)
    R = np.array([[cy * cz, -cx * sz + sx * sy * cz, sx * sz + cx * sy * cz], [cy * sz, cx * cz + sx * sy * sz, -sx * cz + cx * sy * sz], [-sy, sx * cy, cx * cy]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, [x, y, z]
    return T


def test_poses_twin_equals_numpy_and_the_graph_conversion():
    rng = np.random.default_rng(11)
    kp = np.c_[rng.uniform(-100, 100, (64, 3)), rng.uniform(-np.pi, np.pi, (64, 1)), rng.uniform(-1.5, 1.5, (64, 1)), rng.uniform(-np.pi, np.pi, (64, 1))].astype(F32)
    kp[:8, 4] = [np.pi / 2 - 1e-3, -np.pi / 2 + 1e-3, np.pi / 2 - 1e-6, -np.pi / 2 + 1e-6, 1.5707, -1.5707, 1.57, -1.57]
    for G in (np.eye(4), rigid([0.01, -0.02, 0.7], [30, -20, 1.5]), rigid([0, 0, np.pi], [-5, 9, 0])):
        got = binding.map_align_poses(G[:3], kp)
        for i in range(len(kp)):
            X = G @ rzryrx_np(kp[i])
            want = pose6_of_np(X)
            # angles near the pitch singularity are ill-conditioned: compare the poses as transforms, and the numbers where they are not
            dp, da = gap(rzryrx_np(got[i]), X)
            assert dp < 1e-5 * max(1.0, np.abs(X[:3, 3]).max()) and da < 1e-6, (i, got[i], want, dp, da)
            if abs(abs(float(kp[i, 4])) - np.pi / 2) > 1e-2:
                assert np.abs(got[i] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (i, got[i], want)
    assert_bit_equal(binding.map_align_poses(np.eye(4)[:3], kp[8:]), np.array([pose6_of_np(rzryrx_np(k)) for k in kp[8:]]), "identity: the conversion alone")
    assert binding.lib().alego_map_align_poses(None, kp.ctypes.data, 1, kp.ctypes.data) == binding.ERR_ARG


def test_align_math_stand_alone(tmp_path):
    """tests/align_math/align_math_check.cpp over csrc/align_math.h, built with AddressSanitizer and UBSan as a program of its own"""
    exe = str(tmp_path / "align_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "align_math", "align_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "align_math ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


_STRETCH = {}


def stretch(p, start, steps):
    if (start, steps) not in _STRETCH:
        _STRETCH[(start, steps)] = oracle_stretch(p, start, steps)
    return _STRETCH[(start, steps)]


@pytest.fixture(scope="module")
def premise():
    """the two lap cases on the reference side: per case (emulation, ground truth)"""
    p = _params(False)
    out = []
    for name, d, s in LAP_CASES:
        out.append((emulate_pair(p, stretch(p, *s), stretch(p, *d)), truth(d[0], s[0])))
    return out


@pytest.mark.parametrize("case", range(len(LAP_CASES)))
def test_the_premise_on_the_reference_side(premise, case):
    """Two oracle-mapped stretches of the lap as source and destination: numpy descriptors, the oracle's loop_icp, the restated consensus.  Case 0 has
    no mirror overlap and every hypothesis is right; in case 1 the last two queries lie where only the mirror place is inside the destination: their
    hypotheses are accepted by the ICP, agree with each other, and are outvoted."""
    name, d, s = LAP_CASES[case]
    em, T_true = premise[case]
    err = table(em, T_true, f"{name}: destination scans {d[0]}..{d[0] + d[1] - 1}, source scans {s[0]}..{s[0] + s[1] - 1}")
    acc = np.array([h["accepted"] for h in em["hyp"]], bool)
    right = (err[:, 0] < POS_TOL) & (err[:, 1] < ANG_TOL)
    assert len(em["hyp"]) == 8 and acc.all(), "every query's first candidate is accepted by the oracle's ICP"
    if case == 0:
        assert right.all() and em["support"] == 8
    else:
        wrong = ~right
        assert 0 < wrong.sum() < right.sum(), "a minority of aliased hypotheses"
        assert (err[wrong, 0] > 5.0).all() and (err[wrong, 1] > 3.0).all(), "seen the other way round"
        assert (em["sup"][right] == right.sum()).all() and (em["sup"][wrong] < right.sum()).all()
        assert em["sup"][wrong].max() >= 2, "the aliased hypotheses agree among themselves: min_support alone would not tell"
    assert em["status"] == 2 and right[em["best"]]
    dp, da = gap(em["T"], T_true)
    print(f"  chosen: hypothesis {em['best']}, {dp:.4f} m {da:.5f} rad from synth.pose(a)^-1 synth.pose(b)")
    assert dp < POS_TOL and da < ANG_TOL, (dp, da)


def test_default_tolerances_are_the_measured_ones(premise):
    """ALEGO_ALIGN_TOL_TRANS / _ROT = 2 A (rounded up to two / three digits) and below B / 2, A and B measured over the two lap cases"""
    A, B = measure_tolerances(premise)
    print(f"A = {A[0]:.4f} m {A[1]:.5f} rad; B = {B[0]:.3f} m {B[1]:.4f} rad; defaults {TOL_T} m {TOL_R} rad")
    assert 2 * A[0] <= TOL_T <= 2 * A[0] * 1.01 + 1e-3 and 2 * A[1] <= TOL_R <= 2 * A[1] * 1.01 + 1e-4, (A, TOL_T, TOL_R)
    assert TOL_T < B[0] / 2 and TOL_R < B[1] / 2, (B, TOL_T, TOL_R)


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def dev_archive(h, slot):
    """a slot's archive as the emulation reads it, taken from the device"""
    nf = h.map_status(slot)[0]
    kfs = [h.map_get_keyframe(j, slot=slot) for j in range(nf)]
    return dict(poses=np.array([k["pose"] for k in kfs], F32).reshape(-1, 6), frame=lambda j: (kfs[j]["corner"], kfs[j]["surf"], kfs[j]["outlier"]))


def check_consensus_twin(r, tol_t, tol_r, min_support, tag):
    """support, inlier, best and status of a device result equal alego_map_align_consensus on the device's own hypotheses, exactly"""
    H = r["hyp"]
    if not any(x["tried"] for x in H):
        assert (r["status"], r["best"], r["support"]) == (0, -1, 0), (tag, r)
        return
    T, pos, fit, acc = [x["T"] for x in H], [x["pos"] for x in H], [x["fitness"] for x in H], [x["accepted"] for x in H]
    sup, best = binding.map_align_consensus(T, pos, fit, acc, tol_t, tol_r)
    assert [x["support"] for x in H] == sup.tolist() and r["best"] == best, (tag, [x["support"] for x in H], sup, r["best"], best)
    assert r["n_accepted"] == sum(acc) and r["support"] == (int(sup[best]) if best >= 0 else 0), (tag, r)
    assert r["status"] == (2 if best >= 0 and sup[best] >= min_support else 1), (tag, r["status"], sup, best)
    for b, x in enumerate(H):   # inlier: agrees with the best one — the twin on the two of them
        want = 0
        if best >= 0 and acc[b]:
            want = 1 if b == best else int(binding.map_align_consensus([T[best], T[b]], [pos[best], pos[b]], [fit[best], fit[b]], [1, 1], tol_t, tol_r)[0][0] == 2)
            want = want if sup[best] >= 1 and (b != best or sup[b] >= 1) else 0
        assert x["inlier"] == want, (tag, b, x["inlier"], want)
    if best >= 0:
        assert_bit_equal(r["T"], np.asarray(H[best]["T"], np.float64)[:3], f"{tag}: the result's T is the best hypothesis widened")


def align(h, pairs, **kw):
    """h.map_align with every hypothesis' query position (the source key pose's xyz) attached"""
    res = h.map_align(pairs, **kw)
    for (s, d), r in zip(pairs, res):
        for x in r["hyp"]:
            x["pos"] = h.map_get_keyframe(x["src_frame"], slot=s)["pose"][:3]
    return res


SEARCH_FRAMES = {0: 1, 1: 2, 2: 5, 3: 40, 5: 5, 64: 40}   # slot: archived frames; slot 64 lies in the second stream group, slot 5 has a frame with no point in range
SEARCH_PAIRS = [(3, 64), (64, 3), (3, 2), (3, 0), (2, 0), (2, 1), (0, 3), (5, 3), (1, 2), (2, 64)]


@pytest.fixture(scope="module")
def search_handle():
    rng = np.random.default_rng(29)
    h = binding.Handle(_params(False), n_slots=128)   # two stream groups of 64
    assert h.stream_groups()[1] == 64, "slot 64 must lie in another stream group than slots 0 .. 5"
    h.map_enable(40, 1 << 15)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    D = {}
    for s, n in SEARCH_FRAMES.items():
        D[s] = _sparse(rng, n)
        if s == 64:   # rotated, slightly redrawn copies of slot 3's frames in another order: close matches with non-zero shifts, and ties
            D[s] = np.array([np.roll(D[3][(7 * j) % 40], j % 60, axis=0) for j in range(40)])
            D[s][::3, 5, 5] ^= 1
            D[s][11] = D[s][10]
        clouds = [cloud_of(x) for x in D[s]]
        if s == 5:
            clouds[2] = np.array([[300.0, 0, 0, 0], [0, -200.0, 1, 0], [90.0, 90.0, 0, 0]], F32)   # nothing within max_range
        add_frames(h, s, clouds, poses=np.c_[rng.uniform(-30, 30, (n, 3)), rng.uniform(-0.05, 0.05, (n, 2)), rng.uniform(-3, 3, (n, 1))].astype(F32))
        assert h.map_status(s)[:2] == (n, 0), s
    yield dict(h=h, D=D)
    h.close()


@pytest.mark.gpu
def test_search_is_the_brute_force_over_the_destination(search_handle):
    """fitness_max = 1e-12 rejects every attempt, so a query tries all its candidates and the hypothesis left behind is the last one's: with n_cand = 1 .. 4
    every rank of every query is compared with the numpy brute force over the destination's la_desc — pruned, brute, and with a budget that splits a pair's queries"""
    h = search_handle["h"]
    first = h.map_align(SEARCH_PAIRS, n_cand=4, fitness_max=1e-12)
    desc = {s: la_desc(h, s)[0] for s in SEARCH_FRAMES}
    for s, n in SEARCH_FRAMES.items():
        assert desc[s].shape[0] == n, "both archives of every pair are described"
    assert not desc[5][2].any() and desc[5][1].any(), "the frame with no point in range"
    want = {}
    for s, d in SEARCH_PAIRS:
        fr = queries_np(SEARCH_FRAMES[s], 8)
        want[(s, d)] = [(int(f),) + candidates_np(desc[d], desc[s][f], 4) for f in fr]
    assert any(len(c[1]) == 0 for c in want[(5, 3)]) and [len(c[1]) for c in want[(2, 0)]] == [1] * 5 and len(want[(0, 3)]) == 1
    assert any((c[3] != 0).any() for c in want[(3, 64)]), "non-zero shifts"

    def check(res, n_cand, tag):
        for (s, d), r in zip(SEARCH_PAIRS, res):
            assert r["n_queries"] == len(want[(s, d)]) and r["status"] in (0, 1) and r["n_accepted"] == 0, (tag, s, d, r["status"])
            for x, (f, ids, dists, shifts) in zip(r["hyp"], want[(s, d)]):
                k = min(n_cand, len(ids))
                assert (x["src_frame"], x["tried"], x["accepted"]) == (f, k, 0), (tag, s, d, f, x["tried"], k)
                got = (x["dst_frame"], x["dist"], x["shift"])
                assert got == ((int(ids[k - 1]), int(dists[k - 1]), int(shifts[k - 1])) if k else (-1, 0, 0)), (tag, s, d, f, got, ids, dists, shifts)
    check(first, 4, "pruned")
    for brute, budget, tag in ((0, 1 << 22, "pruned"), (1, 1 << 22, "brute"), (0, 50, "a budget that splits a pair's queries"), (1, 1, "brute, one query per chunk")):
        h.set_option("ALEGO_RL_BRUTE", brute)
        h.set_option("ALEGO_RL_BUDGET", budget)
        for n_cand in (1, 2, 3, 4):
            check(h.map_align(SEARCH_PAIRS, n_cand=n_cand, fitness_max=1e-12), n_cand, f"{tag}, n_cand {n_cand}")
    h.set_option("ALEGO_RL_BRUTE", 0)
    h.set_option("ALEGO_RL_BUDGET", 1 << 22)
    # a pair's result does not depend on the other pairs, their order or the ICP chunking
    h.set_option("ALEGO_LC_BUDGET", 1)
    rev = h.map_align(SEARCH_PAIRS[::-1], n_cand=4, fitness_max=1e-12)[::-1]
    h.set_option("ALEGO_LC_BUDGET", 1 << 21)
    for i, pr in enumerate(SEARCH_PAIRS):
        alone = h.map_align([pr], n_cand=4, fitness_max=1e-12)[0]
        for other, tag in ((rev[i], "reversed and chunked"), (alone, "alone")):
            for k in ("status", "n_queries", "n_accepted", "best", "support", "T"):
                assert_bit_equal(np.asarray(other[k]), np.asarray(first[i][k]), f"{pr} {tag}: {k}")
            for a, b in zip(other["hyp"], first[i]["hyp"]):
                for k in a:
                    assert_bit_equal(np.asarray(a[k]), np.asarray(b[k]), f"{pr} {tag}: hyp {k}")


@pytest.mark.gpu
def test_consensus_on_the_device_is_the_twin(search_handle):
    """fitness_max = 1e9 accepts every converged attempt; tolerances from the defaults to ones under which everything agrees"""
    h = search_handle["h"]
    seen = set()
    for tt, tr, ms in ((0.0, 0.0, 0), (5.0, 0.5, 2), (60.0, 2.0, 3), (1e6, 4.0, 1)):
        res = align(h, SEARCH_PAIRS, n_cand=2, fitness_max=1e9, tol_trans=tt, tol_rot=tr, min_support=ms)
        for pr, r in zip(SEARCH_PAIRS, res):
            check_consensus_twin(r, tt, tr, ms if ms > 0 else 2, f"{pr} tol {tt} {tr}")
            seen.add((r["status"], min(r["support"], 3)))
    print("statuses and supports seen:", sorted(seen))
    assert {s for s, _ in seen} >= {1, 2} and any(k >= 2 for _, k in seen), seen


ATT_FRAMES = 8


def attempt_archives():
    """destination: 8 frames, some without a corner or an outlier cloud; source: 3 frames, frame 0 / 2 = destination frame 0 / 7 turned, one bin in twenty redrawn"""
    rng = np.random.default_rng(31)
    kp = lambda n: np.c_[rng.uniform(-30, 30, (n, 3)), rng.uniform(-0.05, 0.05, (n, 2)), rng.uniform(-3, 3, (n, 1))].astype(F32)
    Dd = _sparse(rng, ATT_FRAMES)
    dst = []
    for f, a in enumerate(cloud_of(D) for D in Dd):
        dst.append((EMPTY, a, EMPTY) if f == 5 else (EMPTY, a[0::2], a[1::2]) if f in (0, 7) else (a[0::2], a[1::2], EMPTY) if f == 2 else split3(a))
    Ds = _sparse(rng, 3)
    for f, (best, turn) in {0: (0, 11), 2: (ATT_FRAMES - 1, 53)}.items():
        q = np.roll(Dd[best], turn, axis=0)
        redraw = rng.random(q.shape) < 0.05
        q[redraw] = rng.integers(1, 256, int(redraw.sum()))
        Ds[f] = q
    src = [split3(cloud_of(D)) for D in Ds]
    src[1] = (EMPTY, src[1][1], src[1][2])
    return (src, kp(3)), (dst, kp(ATT_FRAMES))


@pytest.mark.gpu
@pytest.mark.parametrize("search_num", [None, 0])
def test_every_attempt_is_the_attempt_on_its_candidate(search_num):
    """fitness_max = 1e-12 rejects every attempt: with n_cand = 1 and 2 the hypothesis left behind is candidate 0's and candidate 1's (a rejected candidate is
    followed by the next), compared with the oracle's loop_icp on the device's own frames; candidates 0 and nd - 1 clamp the window at both ends"""
    p = _params(False) if search_num is None else _params(False, lc_search_num=search_num)
    (src, kps), (dst, kpd) = attempt_archives()
    h = binding.Handle(p, n_slots=2)
    h.map_enable(16, 1 << 14)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    for s, (fr, kp) in enumerate(((src, kps), (dst, kpd))):
        for f in range(len(fr)):
            h.lm_add_keyframe(kp[f], *fr[f], slot=s)
    S, Dv = dev_archive(h, 0), dev_archive(h, 1)
    assert_bit_equal(Dv["poses"], kpd, "the archived destination poses")
    nd = ATT_FRAMES
    firsts = set()
    for n_cand in (1, 2):
        em = emulate_pair(p, S, Dv, n_cand=n_cand, fitness_max=1e-12)
        r = h.map_align([(0, 1)], n_cand=n_cand, fitness_max=1e-12)[0]
        assert r["n_queries"] == 3 and r["status"] == 1 and r["best"] == -1 and r["n_accepted"] == 0, r
        for x, e in zip(r["hyp"], em["hyp"]):
            tag = f"lc_search_num {p.lc_search_num}, n_cand {n_cand}, source frame {e['src_frame']}"
            want = e["want"]
            assert (x["src_frame"], x["tried"], x["accepted"], x["dst_frame"], x["dist"], x["shift"]) == (e["src_frame"], n_cand, 0, e["dst_frame"], e["dist"], e["shift"]), (tag, x, e)
            if n_cand == 1:
                firsts.add(x["dst_frame"])
            print(f"{tag}: candidate {x['dst_frame']} shift {x['shift']}; device: n_source {x['n_source']} n_target {x['n_target']} converged {x['converged']} iterations {x['iterations']} "
                  f"fitness {x['fitness']:.9g}; oracle: {want['n_source']} {want['n_target']} {want['converged']} {want['iterations']} {want['fitness']:.9g}")
            assert_bit_equal(x["guess6"], guess_of(kpd, x["dst_frame"], x["shift"]), f"{tag}: guess6")
            assert (x["n_source"], x["n_target"], x["converged"]) == (want["n_source"], want["n_target"], want["converged"]), (tag, x, want)
            assert x["n_source"] == sum(len(c) for c in src[e["src_frame"]]) and x["n_target"] > 0, tag
            assert abs(x["iterations"] - want["iterations"]) <= 1, (tag, x["iterations"], want["iterations"])
            assert np.abs(x["icp_final"] - want["T"]).max() < 1e-5, (tag, x["icp_final"], want["T"])
            assert abs(x["fitness"] - want["fitness"]) < 1e-6 * max(1.0, want["fitness"]), (tag, x["fitness"], want["fitness"])
            assert np.abs(x["T"] - e["T"]).max() < 1e-5 * max(1.0, np.abs(e["T"][:3, 3]).max()), (tag, x["T"], e["T"])
    assert {0, nd - 1} <= firsts, f"candidates 0 and nd - 1 are tried: {firsts}"
    h.close()


LAP_SLOT = {(0, 251): 0, (100, 171): 1, (100, 431): 2}


@pytest.fixture(scope="module")
def lap_handle():
    """one slot per stretch of LAP_CASES, every scan through alego_scan_process"""
    p = _params(False)
    h = binding.Handle(p, n_slots=3)
    h.map_enable(64, 1 << 19)
    h.graph_enable(4)   # records the chain edges; nothing is optimised or applied before the test of the state, which runs last on this handle
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    from test_loop_search import _scan
    for (start, steps), s in LAP_SLOT.items():
        for k in range(steps):
            h.scan_process(_scan(p, (start + k) % LAP), stages=7, slot=s, stamp=0.1 * k)
        assert h.map_status(s)[1] == 0 and h.map_status(s)[0] > 10, (s, h.map_status(s))
    yield dict(p=p, h=h)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(LAP_CASES)))
def test_lap_cases_against_the_emulation(lap_handle, case):
    p, h = lap_handle["p"], lap_handle["h"]
    name, d, s = LAP_CASES[case]
    sd, ss = LAP_SLOT[d], LAP_SLOT[s]
    r = align(h, [(ss, sd)])[0]
    em = emulate_pair(p, dev_archive(h, ss), dev_archive(h, sd))
    T_true = truth(d[0], s[0])
    err = table(em, T_true, f"{name} (the emulation on the device's archives)")
    assert r["n_queries"] == len(em["hyp"]) == 8
    for q, (x, e) in enumerate(zip(r["hyp"], em["hyp"])):
        assert (x["src_frame"], x["dst_frame"], x["dist"], x["shift"], x["tried"], x["accepted"]) == (e["src_frame"], e["dst_frame"], e["dist"], e["shift"], e["tried"], e["accepted"]), (q, x, e)
        assert x["support"] == em["sup"][q], (q, x["support"], em["sup"])
    assert (r["status"], r["best"], r["support"]) == (em["status"], em["best"], em["support"]) == (2, em["best"], 8 if case == 0 else em["support"]), (r, em["status"], em["best"])
    assert np.abs(full(r["T"]) - em["T"]).max() < 1e-5 * max(1.0, np.abs(em["T"][:3, 3]).max()), (r["T"], em["T"])
    dp, da = gap(r["T"], T_true)
    print(f"  device: best {r['best']} support {r['support']}; {dp:.4f} m {da:.5f} rad from the truth")
    assert dp < POS_TOL and da < ANG_TOL, (dp, da)
    if case == 1:
        wrong = (err[:, 0] > 5.0) & (err[:, 1] > 3.0)
        assert 0 < wrong.sum() < 4 and [x["inlier"] for x in r["hyp"]] == [0 if w else 1 for w in wrong], (wrong, [x["inlier"] for x in r["hyp"]])
    check_consensus_twin(r, TOL_T, TOL_R, 2, name)


@pytest.mark.gpu
def test_moved_archive(lap_handle):
    """the source archive moved by a known rigid G (alego_map_align_poses + alego_map_set_keyposes): the new T is T G^-1"""
    h = lap_handle["h"]
    ss, sd = LAP_SLOT[(100, 171)], LAP_SLOT[(0, 251)]
    r0 = h.map_align([(ss, sd)])[0]
    kp = dev_archive(h, ss)["poses"]
    G = rigid([0.01, -0.02, 0.7], [30, -20, 1.5])
    h.map_set_keyposes(0, binding.map_align_poses(G[:3], kp), slot=ss)
    r1 = h.map_align([(ss, sd)])[0]
    h.map_set_keyposes(0, kp, slot=ss)
    r2 = h.map_align([(ss, sd)])[0]
    want = full(r0["T"]) @ inv(G)
    assert (r1["status"], r1["best"], r1["support"]) == (r0["status"], r0["best"], r0["support"]) == (2, r0["best"], 8), (r0, r1)
    assert np.abs(full(r1["T"]) - want).max() < 1e-5 * max(1.0, np.abs(want[:3, 3]).max()), (r1["T"], want)
    assert np.abs(want[:3, 3] - r0["T"][:, 3]).max() > 5.0, "G moved the archive"
    for k in ("status", "best", "support", "T"):
        assert_bit_equal(np.asarray(r2[k]), np.asarray(r0[k]), f"the poses put back: {k}")


@pytest.mark.gpu
def test_align_changes_no_device_state_and_no_existing_result(lap_handle):
    """lm_state, lm_info, the archive, stamps, key poses, map_status and the key-pose graph (status, chain edges, loop edges, the last estimate) are byte-equal
    around a call; both loop searches return the same bytes before and after it"""
    h = lap_handle["h"]
    ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
    for s in range(3):   # a graph with something in every part: one loop edge per slot (loop_closed_ set) and an estimate, nothing applied
        h.graph_add_edge(h.map_status(s)[0] - 1, 0, rigid([0.0, 0.0, 0.1], [1.0, -2.0, 0.0])[:3], np.full(6, 0.5), slot=s)
    assert all(g["status"] in (1, 2) and g["applied"] == 0 for g in h.graph_optimize([0, 1, 2], apply=False))

    def graph(s):
        st = h.graph_status(s)
        assert st[0] == h.map_status(s)[0] and st[1] == 1 and st[2] == 1 and st[3] == st[0], (s, st)
        ch, lp = h.graph_get_edges(kind=0, slot=s), h.graph_get_edges(kind=1, slot=s)
        return [np.array(st)] + [e[k] for e in (ch, lp) for k in ("frm", "to", "between", "variance")] + [h.graph_get_estimate(slot=s)]
    WHAT = ("lm_state", "lm_info", "the archive", "stamps", "key poses", "map_status", "graph_status") + tuple(f"{e} edges: {k}" for e in ("chain", "loop") for k in ("from", "to", "between", "variance")) + ("the graph's estimate",)
    snap = lambda s: [h.debug_get("lm_state", slot=s), h.debug_get("lm_info", slot=s), h.map_assemble(ALL, slot=s), h.map_get_stamps(slot=s),
                      np.array([h.map_get_keyframe(j, slot=s)["pose"] for j in range(h.map_status(s)[0])], F32), np.array(h.map_status(s))] + graph(s)
    flat = lambda res: [np.asarray(r[k]) for r in res for k in sorted(r)]
    radius, app = flat(h.loop_search([0, 1, 2])), flat(h.loop_search_appearance([0, 1, 2]))
    before = [snap(s) for s in range(3)]
    res = h.map_align([(1, 0), (2, 0), (0, 2)])
    assert [r["status"] for r in res] == [2, 2, 2], "the call did its work"
    after = [snap(s) for s in range(3)]
    for b, a in zip(before, after):
        assert len(b) == len(a) == len(WHAT)
        for x, y, what in zip(b, a, WHAT):
            assert_bit_equal(np.asarray(x), np.asarray(y), what)
    for x, y in zip(radius, flat(h.loop_search([0, 1, 2]))):
        assert_bit_equal(x, y, "alego_loop_search after alego_map_align")
    for x, y in zip(app, flat(h.loop_search_appearance([0, 1, 2]))):
        assert_bit_equal(x, y, "alego_loop_search_appearance after alego_map_align")


@pytest.mark.gpu
def test_align_boundaries():
    p = _params(False)
    rng = np.random.default_rng(3)
    h = binding.Handle(p, n_slots=4)
    h.map_enable(3, 1 << 12)
    with pytest.raises(binding.AlegoError):
        h.map_align([(0, 1)])                 # the search is not enabled
    h.loop_appearance_enable()
    for bad in ([(0, 4)], [(-1, 0)], [(1, 1)], [(0, 1), (2, 3), (0, 1)]):
        with pytest.raises(binding.AlegoError):
            h.map_align(bad)
    with pytest.raises(binding.AlegoError):
        h.map_align([(0, 1)], n_queries=33)
    with pytest.raises(binding.AlegoError):
        h.map_align([(0, 1)], n_cand=9)
    assert h.map_align([]) == []
    assert [(r["status"], r["n_queries"], r["best"]) for r in h.map_align([(0, 1), (1, 0)])] == [(0, 0, -1)] * 2, "both archives empty"
    clouds = [cloud_of(D) for D in _sparse(rng, 5)]
    add_frames(h, 0, clouds[:1])
    add_frames(h, 2, clouds[:2])
    add_frames(h, 3, clouds)                  # five frames into an archive of three: two dropped
    assert h.map_status(3)[1] > 0
    res = h.map_align([(0, 1), (1, 0), (0, 3), (3, 2), (0, 2), (2, 0)], fitness_max=1e9)
    assert [r["status"] for r in res[:4]] == [0, 0, -1, -1], [r["status"] for r in res]
    one = res[4]                              # ns = 1: Q = 1 and, with min_support 2, status 1
    assert one["n_queries"] == 1 and one["hyp"][0]["src_frame"] == 0 and one["hyp"][0]["tried"] >= 1
    assert one["status"] == 1 and one["support"] == one["n_accepted"] <= 1, one
    assert res[5]["n_queries"] == 2
    if one["n_accepted"] == 1:
        assert h.map_align([(0, 2)], fitness_max=1e9, min_support=1)[0]["status"] == 2
    # hyp == NULL and opts == NULL
    out = (binding.MapAlignResult * 2)()
    src, dst = np.array([0, 0], np.int32), np.array([2, 3], np.int32)
    assert binding.lib().alego_map_align(h._h, src.ctypes.data, dst.ctypes.data, 2, None, out, None) == 0 and out[1].status == -1 and out[0].n_queries == 1
    assert [r["status"] for r in h.map_align([(0, 2), (0, 3)], hyps=False)] == [out[0].status, -1]
    h.close()
    # a localising handle
    h = binding.Handle(p, n_slots=2)
    h.loc_enable([(np.zeros(6, F32), EMPTY, EMPTY, EMPTY)], 0.0)
    with pytest.raises(binding.AlegoError, match="alego_map_align: not available on a localising handle"):
        h.map_align([(0, 1)])             # a valid pair of two slots in range: only the handle is at fault
    h.close()


@pytest.mark.gpu
def test_replay_align_agrees_with_the_binding():
    """examples/replay N --align START2: slot 1 replays the lap START2 scans further on; its last line is alego_map_align(1 -> 0) with the defaults"""
    from test_loop_search import _scan
    n, start2 = 150, 30   # scans 0 .. 149 and 30 .. 179: most of the source lies inside the destination, and no mirror place (s +- 280) does
    exe = os.path.join(ROOT, "examples", "replay")
    out = subprocess.run([exe, str(n), "--align", str(start2)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("align:")]
    p = synth.default_params(16, 1800)
    h = binding.Handle(p, n_slots=2)
    h.map_enable(4096, 1 << 24)
    h.loop_appearance_enable()
    for k in range(n):
        h.scan_process(_scan(p, k), stages=7, slot=0, stamp=0.1 * k)
        h.scan_process(_scan(p, start2 + k), stages=7, slot=1, stamp=0.1 * k)
    r = h.map_align([(1, 0)], hyps=False)[0]
    h.close()
    want = f"align: status {r['status']} queries {r['n_queries']} accepted {r['n_accepted']} support {r['support']} T" + "".join(f" {v:.9g}" for v in np.asarray(r["T"]).reshape(12))
    print("\n".join(got))
    assert got == [want], (got, want)
    dp, da = gap(r["T"], truth(0, start2))
    assert r["status"] == 2 and dp < POS_TOL and da < ANG_TOL, (r, dp, da)
