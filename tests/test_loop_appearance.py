"""Loop closures by appearance (alego_loop_appearance_enable / alego_loop_search_appearance, kernels_reloc.hip): a SLAM
slot's newest archived frame is searched among the older frames of its own archive with the descriptor, the exact search and the
yaw-shifted guess of relocalisation, and verified by the ICP of alego_loop_search.

References: the numpy restatements of tests/test_relocalize.py (descriptor, match over all 60 shifts, guess), a numpy brute force of the
eligibility and candidate rule, the host twin alego_loop_appearance_candidates, and the UNCHANGED oracle's loop_detect / loop_icp run on the
device's own archive (as tests/test_loop_search.py::device_ref does).

Drift is imitated by moving archived key poses along a ramp (RAMP_FROM, RAMP_END): frame i moves by w_i * (60, -35, 2) m and w_i * 0.5 rad of
yaw, w_i = max(0, (i - 30) / (n - 1 - 30)), so the newest frame ends 69.5 m from where it stood.  alego_map_set_keyposes moves the ARCHIVE
only: a slot's t_map2laser_, which alego_loop_search measures its radius from, stays where the last mapping frame left it until the next
mapping frame recomputes it.  The radius rule on the drifted poses is therefore judged where drift puts the robot — at the
moved newest key pose — with alego_loop_detect and the oracle's loop_detect on the device's archive; alego_loop_search itself is checked
against the oracle's verdict on the state it really reads.
"""
import os
import re

import numpy as np
import pytest

from alego_amd import binding, synth
from test_loop_search import _initial_guess, _params, _scan, device_ref, oracle_replay, replay_handle
from test_relocalize import ANG_TOL, POS_TOL, constructed_clouds, desc_np, guess_of, match_all_np
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAP = 560
NS, NR = 60, 20
NEW_SYMBOLS = ["alego_loop_appearance_enable", "alego_loop_search_appearance", "alego_loop_appearance_candidates"]
MAX_RANGE, Z_OFFSET = 80.0, 4.0   # the defaults, spelt out
RAMP_FROM, RAMP_END = 30, np.array([60.0, -35.0, 2.0, 0.5])
EMPTY = np.zeros((0, 4), F32)


def _O():
    from oracle import oracle_py
    return oracle_py


# ---- the rule in numpy ----------------------------------------------------------------------------------------------------------
def eligible_np(kp, stamps, gap, max_jump):
    """eligibility of frames 0 .. n - 2 for the query n - 1"""
    kp = np.asarray(kp, F32).reshape(-1, 6)
    st = np.asarray(stamps, np.float64)
    n = len(kp)
    el = st[n - 1] - st[:n - 1] > gap
    if max_jump > 0:
        d = kp[:n - 1, :3] - kp[n - 1, :3]
        d2 = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == F32
        el &= d2 < F32(max_jump * max_jump)
    return el


def candidates_np(desc, kp, stamps, gap, max_jump=0.0, max_dist=0, n_cand=4):
    """(ids, dists, shifts, eligible count): the brute force over every eligible frame and all 60 shifts"""
    desc = np.asarray(desc, np.uint8).reshape(-1, NS, NR)
    n = len(desc)
    none = (np.zeros(0, np.int32),) * 3
    if n < 2:
        return none + (0,)
    if not desc[n - 1].any():
        return none + (0,)   # an empty query descriptor has no eligible frame
    el = np.nonzero(eligible_np(kp, stamps, gap, max_jump))[0]
    if len(el) == 0:
        return none + (0,)
    d, s = match_all_np(desc[el], desc[n - 1])
    order = np.lexsort((el, d))[:n_cand]
    if max_dist > 0:
        order = order[d[order] <= max_dist]
    return el[order].astype(np.int32), d[order].astype(np.int32), s[order].astype(np.int32), len(el)


def ramp(kp):
    """the drifted key poses"""
    out = np.array(kp, F32).reshape(-1, 6).copy()
    n = len(out)
    for i in range(n):
        w = max(0.0, (i - RAMP_FROM) / max(1, n - 1 - RAMP_FROM))
        out[i, :3] += F32(w) * RAMP_END[:3].astype(F32)
        out[i, 5] += F32(0.5 * w)
    return out


def pose_gap(T, pose6):
    """(m, rad) between the 4 x 4 T and matrix(pose6)"""
    G = _initial_guess(np.asarray(pose6, F32)).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(4, 4)
    c = (np.trace(G[:3, :3].T @ T[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(T[:3, 3] - G[:3, 3])), float(np.arccos(np.clip(c, -1.0, 1.0)))


def emulate(p, kp, frame, i, s):
    """the oracle's loop_icp on candidate (i, s) of the newest frame: (result, guess6, t_correct, between)"""
    n = len(kp)
    g = guess_of(kp, i, s)
    fr = [(g,) + tuple(frame(n - 1))]
    for j in range(i - p.lc_search_num, i + p.lc_search_num + 1):
        if 0 <= j < n - 1:
            fr.append((kp[j],) + tuple(frame(j)))
    want, _ = _O().loop_icp(p, fr)
    t_correct, between = binding.loop_constraint(want["T"], g, kp[i])
    return want, g, np.asarray(t_correct, F32).reshape(4, 4), np.asarray(between, np.float64).reshape(3, 4)


def world_correction_np(t_correct, latest6):
    G = _initial_guess(np.asarray(latest6, F32)).astype(np.float64)
    Gi = np.eye(4)
    Gi[:3, :3] = G[:3, :3].T
    Gi[:3, 3] = -G[:3, :3].T @ G[:3, 3]
    return np.asarray(t_correct, np.float64).reshape(4, 4) @ Gi


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_appearance_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s
    assert "alego_loop_app_opts" in hdr and "alego_loop_app_info" in hdr


def _sparse(rng, n):
    return (rng.integers(0, 256, (n, NS, NR)) * (rng.random((n, NS, NR)) < 0.3)).astype(np.uint8)


def twin_cases():
    """(name, desc (n, 60, 20), keyposes (n, 6), stamps (n,), gap, max_jump, max_dist, n_cand)"""
    rng = np.random.default_rng(41)
    kp = lambda n: np.c_[rng.uniform(-30, 30, (n, 3)), rng.uniform(-3, 3, (n, 3))].astype(F32)
    lin = lambda n: np.arange(n) * 10.0
    out = []
    out.append(("random sparse", _sparse(rng, 40), kp(40), lin(40), 30.0, 0.0, 0, 4))
    out.append(("random sparse, n_cand 8", _sparse(rng, 40), kp(40), lin(40), 30.0, 0.0, 0, 8))
    out.append(("n = 0", _sparse(rng, 0), kp(0), lin(0), 30.0, 0.0, 0, 4))
    out.append(("n = 1", _sparse(rng, 1), kp(1), lin(1), 30.0, 0.0, 0, 4))
    out.append(("n = 2", _sparse(rng, 2), kp(2), np.array([0.0, 31.0]), 30.0, 0.0, 0, 4))
    out.append(("fewer eligible than n_cand", _sparse(rng, 12), kp(12), np.r_[0.0, 5.0, 8.0, 100.0 + np.arange(9)], 30.0, 0.0, 0, 4))
    out.append(("no eligible frame", _sparse(rng, 12), kp(12), np.arange(12) * 1.0, 30.0, 0.0, 0, 4))
    st = lin(30)
    body = st[:29].copy()
    rng.shuffle(body)
    out.append(("shuffled stamps: not a prefix", _sparse(rng, 30), kp(30), np.r_[body, st[29]], 95.0, 0.0, 0, 4))
    out.append(("a gap of exactly min_time_gap is not eligible", _sparse(rng, 6), kp(6), np.array([0.0, 69.5, 70.0, 70.0, 80.0, 100.0]), 30.0, 0.0, 0, 8))
    k = kp(9)
    k[:, :3] = 0
    k[:8, 0] = [3.0, 4.0, 5.0, 5.0, 4.999999, 5.000001, 0.0, -5.0]
    k[3, :3] = [3.0, 4.0, 0.0]   # d2 = 9 + 16 = 25 exactly
    out.append(("d2 equal to max_jump^2 exactly is not eligible", _sparse(rng, 9), k, lin(9) * 10, 30.0, 5.0, 0, 8))
    base = _sparse(rng, 5)
    out.append(("ties in D broken by id", np.concatenate([base[[1, 0, 1, 0, 2, 2, 1]], np.roll(base[:1], 9, axis=1)]), kp(8), lin(8) * 10, 30.0, 0.0, 0, 4))
    out.append(("identical frames", np.repeat(base[3:4], 10, axis=0), kp(10), lin(10) * 10, 30.0, 0.0, 0, 4))
    d = _sparse(rng, 40)
    d[7] = np.roll(d[39], -5, axis=0)
    d[11] = np.roll(d[39], -50, axis=0)
    d[11, 0, 0] ^= 3
    out.append(("the max_dist cut", d, kp(40), lin(40) * 10, 30.0, 0.0, 100, 4))
    z = _sparse(rng, 10)
    z[9] = 0
    out.append(("all-zero newest frame", z, kp(10), lin(10) * 10, 30.0, 0.0, 0, 4))
    return out


@pytest.mark.parametrize("case", range(len(twin_cases())))
def test_candidates_twin_equals_numpy(case):
    name, desc, kp, st, gap, mj, md, nc = twin_cases()[case]
    got = binding.loop_appearance_candidates(desc, kp, st, gap, mj, md, nc)
    want = candidates_np(desc, kp, st, gap, mj, md, nc)
    for g, w, what in zip(got, want, ("ids", "dists", "shifts")):
        assert np.array_equal(g, w), (name, what, g, w)
    n = len(desc)
    if name.startswith("n = 0") or name.startswith("n = 1") or name.startswith("no eligible") or name.startswith("all-zero"):
        assert len(got[0]) == 0
    if name.startswith("n = 2"):
        assert got[0].tolist() == [0]
    if name.startswith("fewer"):
        assert sorted(got[0].tolist()) == [0, 1, 2]
    if name.startswith("shuffled"):
        el = eligible_np(kp, st, gap, mj)
        assert 0 < el.sum() < n - 1 and not el[:el.sum()].all(), "eligibility must not be a prefix"
        assert el[got[0]].all()
    if name.startswith("a gap of exactly"):
        assert sorted(got[0].tolist()) == [0, 1]
    if name.startswith("d2 equal"):
        assert sorted(got[0].tolist()) == [0, 1, 4, 6], got[0]   # 3 and 4 m, just below 5 m, the origin; 5 m three times and just above are out
    if name.startswith("ties"):
        assert (np.diff(got[1]) == 0).any() and (np.diff(got[0])[np.diff(got[1]) == 0] > 0).all()
        assert got[0][0] == 1 or got[1][0] == 0
    if name.startswith("identical"):
        assert got[0].tolist() == [0, 1, 2, 3] and not got[1].any() and not got[2].any()
    if name.startswith("the max_dist"):
        assert got[0].tolist() == [7, 11] and got[1][0] == 0 and 0 < got[1][1] <= 100 and got[2].tolist() == [5, 50]
    L = binding.lib()
    i3 = np.zeros(8, np.int32)
    assert L.alego_loop_appearance_candidates(None, None, None, 3, 30.0, 0.0, 0, 4, i3.ctypes.data, i3.ctypes.data, i3.ctypes.data) == binding.ERR_ARG
    assert L.alego_loop_appearance_candidates(None, None, None, 0, 30.0, 0.0, 0, 9, i3.ctypes.data, i3.ctypes.data, i3.ctypes.data) == binding.ERR_ARG


@pytest.mark.parametrize("start", [0, 333])
def test_the_premise_on_the_reference_side(start):
    """The lap mapped by the oracle for 556 scans; frames above 30 moved by the ramp.  The radius rule finds a frame on the unmoved poses and
    none on the moved ones; numpy candidates + the oracle's loop_icp accept candidate 0 and put the newest frame back where it stood."""
    O = _O()
    p = _params(False)
    ref = oracle_replay(p, start, 556)
    o, kp, stamps = ref["o"], ref["poses"].astype(F32), ref["stamps"]
    n = len(kp)
    frames = [o.lm_keyframe(i) for i in range(n)]
    o.close()
    desc = np.array([desc_np(np.concatenate(f), MAX_RANGE, Z_OFFSET)[0] for f in frames])
    kpd = ramp(kp)
    assert np.linalg.norm(kpd[-1, :3] - kp[-1, :3]) > 3 * p.lc_search_radius
    assert O.loop_detect(p, kp, stamps, kp[-1, :3].astype(np.float64)) >= 0, "the radius rule finds the revisit while the poses are right"
    assert O.loop_detect(p, kpd, stamps, kpd[-1, :3].astype(np.float64)) == -1, "and nothing once the drift exceeds the radius"
    assert binding.loop_detect(p, kpd, stamps, kpd[-1, :3].astype(np.float64)) == -1
    ids, dists, shifts, nel = candidates_np(desc, kpd, stamps, p.lc_min_time_gap, n_cand=2)
    i0, s0 = int(ids[0]), int(shifts[0])
    # the condition of the accuracy below: no frame of the target sub-map is moved
    assert i0 + p.lc_search_num + 1 < RAMP_FROM + 1 and np.array_equal(kpd[:i0 + p.lc_search_num + 1], kp[:i0 + p.lc_search_num + 1])
    want, g, t_correct, _ = emulate(p, kpd, lambda j: frames[j], i0, s0)
    dp, da = pose_gap(t_correct, kp[-1])
    print(f"start {start}: {n} frames, {nel} eligible, frame {i0} D {dists[0]} (next: frame {ids[1]} D {dists[1]}) shift {s0} iterations {want['iterations']} "
          f"fitness {want['fitness']:.4f}; t_correct {dp:.4f} m {da:.5f} rad from the unmoved newest pose")
    assert want["converged"] and want["fitness"] <= p.lc_fitness_max, want
    assert dp < POS_TOL and da < ANG_TOL, (dp, da)


@pytest.mark.parametrize("start", [0, 37, 333])
def test_aliased_candidates_on_the_reference_side(start):
    """470 scans: no revisit yet.  The world is symmetric under a half turn, and the best candidate is a frame seen the other way round, which the
    oracle's ICP accepts under lc_fitness_max: what the gates of the search are for (DESIGN.md section 16 carries the printed rows)."""
    p = _params(False)
    ref = oracle_replay(p, start, 470)
    o, kp, stamps = ref["o"], ref["poses"].astype(F32), ref["stamps"]
    n = len(kp)
    frames = [o.lm_keyframe(i) for i in range(n)]
    o.close()
    desc = np.array([desc_np(np.concatenate(f), MAX_RANGE, Z_OFFSET)[0] for f in frames])
    kpd = ramp(kp)
    ids, dists, shifts, nel = candidates_np(desc, kpd, stamps, p.lc_min_time_gap, n_cand=1)
    want, g, t_correct, _ = emulate(p, kpd, lambda j: frames[j], int(ids[0]), int(shifts[0]))
    dp, da = pose_gap(t_correct, kp[-1])
    print(f"470 scans from {start}: {n} frames, {nel} eligible, frame {ids[0]} D {dists[0]} shift {shifts[0]} iterations {want['iterations']} fitness {want['fitness']:.4f}; "
          f"t_correct {dp:.1f} m {da:.3f} rad from the unmoved newest pose")
    assert want["converged"] and want["fitness"] <= p.lc_fitness_max and dp > 5.0 and da > 3.0, (want, dp, da)
    jump = float(np.linalg.norm(kpd[ids[0], :3] - kpd[-1, :3]))
    assert len(candidates_np(desc, kpd, stamps, p.lc_min_time_gap, max_jump=0.5 * jump, n_cand=1)[0]) == 0, "max_jump below the jump leaves no candidate"


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _pts(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.c_[xyz, np.zeros(len(xyz))].astype(F32)


def cloud_of(D, max_range=MAX_RANGE, z_offset=Z_OFFSET):
    """a cloud with one point per non-zero bin of D (60, 20), in the middle of the bin, whose descriptor is D"""
    sec, ring = np.nonzero(D)
    w = max_range / 20.0
    r = (ring + 0.5) * w
    a = (sec + 0.5) * (2.0 * np.pi / 60.0) - np.pi
    z = (D[sec, ring].astype(np.float64) - 0.5) / 16.0 - z_offset
    return _pts(np.c_[r * np.cos(a), r * np.sin(a), z])


def split3(a):
    return a[0::3], a[1::3], a[2::3]


def add_frames(h, slot, clouds, poses=None, first=0):
    for k, c in enumerate(clouds):
        pose = np.array([first + k, 0, 0, 0, 0, 0], F32) if poses is None else np.asarray(poses[k], F32)
        corner, surf, outl = split3(np.ascontiguousarray(c, F32).reshape(-1, 4))
        h.lm_add_keyframe(pose, corner, surf, outl, slot=slot)


def la_desc(h, slot):
    return h.debug_get("la_desc", slot=slot).reshape(-1, NS, NR), h.debug_get("la_key", slot=slot).view(np.uint16).reshape(-1, NR)


@pytest.mark.gpu
def test_device_descriptors_are_the_numpy_rule():
    rng = np.random.default_rng(7)
    p = _params(False)
    cases = [c for c in constructed_clouds() if c[2] == 40.0 and c[3] == 4.0]
    assert len(cases) >= 6 and any(c[0] == "empty" for c in cases)
    clouds = [c[1] for c in cases] + [cloud_of(D, 40.0, 4.0) for D in _sparse(rng, 3)]
    MAXF = len(clouds) + 4
    h = binding.Handle(p, n_slots=2)
    h.map_enable(MAXF, 1 << 16)
    with pytest.raises(binding.AlegoError):
        h.debug_get("la_desc")
    h.loop_appearance_enable(40.0, 4.0)
    assert la_desc(h, 0)[0].shape[0] == 0, "nothing is described before a search"
    add_frames(h, 0, clouds)
    add_frames(h, 1, clouds[:2])
    h.loop_search_appearance([0], verify=0)
    want = np.array([desc_np(c, 40.0, 4.0)[0] for c in clouds])
    got, keys = la_desc(h, 0)
    assert got.shape[0] == len(clouds)
    for i in range(len(clouds)):
        assert np.array_equal(got[i], want[i]), (i, np.argwhere(got[i] != want[i])[:5])
    assert np.array_equal(keys, want.astype(np.int64).sum(axis=1))
    assert np.array_equal(want[-3:], _sparse(np.random.default_rng(7), 3)), "one point per wanted bin gives the wanted descriptor"
    assert la_desc(h, 1)[0].shape[0] == 0, "an unlisted slot is not described"
    # frames appended later are picked up by the next search; the rows described before stay as they are
    more = [cloud_of(D, 40.0, 4.0) for D in _sparse(rng, 4)]
    add_frames(h, 0, more, first=len(clouds))
    assert h.map_status(0)[0] == MAXF and h.map_status(0)[1] == 0
    h.loop_search_appearance([0, 1], verify=0)
    got2, keys2 = la_desc(h, 0)
    assert got2.shape[0] == MAXF and np.array_equal(got2[:len(clouds)], got) and np.array_equal(keys2[:len(clouds)], keys)
    want2 = np.array([desc_np(c, 40.0, 4.0)[0] for c in more])
    assert np.array_equal(got2[len(clouds):], want2), "the frame at index max_keyframes - 1 is described"
    assert np.array_equal(la_desc(h, 1)[0], want[:2])
    # key poses are not part of a descriptor
    h.map_set_keyposes(0, np.tile(np.array([5, 6, 7, 0.1, 0.2, 0.3], F32), (MAXF, 1)), slot=0)
    h.loop_search_appearance([0], verify=0)
    got3, keys3 = la_desc(h, 0)
    assert np.array_equal(got3, got2) and np.array_equal(keys3, keys2)
    h.close()


N_CAND = 4


def search_slots():
    """per slot: (name, descriptors (n, 60, 20), key poses (n, 6), stamps (n,) or None for the archive's own, max_jump, max_dist)"""
    rng = np.random.default_rng(19)
    kp = lambda n: np.c_[rng.uniform(-30, 30, (n, 3)), rng.uniform(-3, 3, (n, 3))].astype(F32)
    far = lambda n: np.arange(n) * 100.0
    out = []
    out.append(("0 frames", _sparse(rng, 0), kp(0), None, 0.0, 0))
    out.append(("1 frame", _sparse(rng, 1), kp(1), far(1), 0.0, 0))
    out.append(("2 frames", _sparse(rng, 2), kp(2), far(2), 0.0, 0))
    out.append(("n_cand frames", _sparse(rng, N_CAND), kp(N_CAND), far(N_CAND), 0.0, 0))
    out.append(("255 frames, all ineligible", _sparse(rng, 255), kp(255), np.arange(255) * 0.1, 0.0, 0))
    st = np.full(256, 1000.0)
    st[77] = 0.0
    out.append(("256 frames, exactly one eligible", _sparse(rng, 256), kp(256), st, 0.0, 0))
    st = np.full(257, 1000.0)
    st[[3, 200, 255]] = [10.0, 20.0, 969.0]
    out.append(("257 frames, n_cand - 1 eligible", _sparse(rng, 257), kp(257), st, 0.0, 0))
    body = np.arange(256) * 1.0
    rng.shuffle(body)
    out.append(("257 frames, eligibility not a prefix", _sparse(rng, 257), kp(257), np.r_[body, 200.0], 0.0, 0))   # eligible: stamps below 170
    base = _sparse(rng, 6)
    dup = np.concatenate([base, base, base[::-1], np.roll(base[:1], 7, axis=1)])
    out.append(("duplicate descriptors", dup, kp(len(dup)), far(len(dup)), 0.0, 0))
    z = _sparse(rng, 20)
    z[19] = 0
    out.append(("an all-zero newest frame", z, kp(20), far(20), 0.0, 0))
    k = kp(60)
    out.append(("max_jump binding", _sparse(rng, 60), k, far(60), 25.0, 0))
    d = _sparse(rng, 60)
    d[13] = np.roll(d[59], -21, axis=0)
    d[40] = np.roll(d[59], -2, axis=0)
    d[40, 5, 5] ^= 1
    out.append(("max_dist binding", d, kp(60), far(60), 0.0, 300))
    return out


@pytest.fixture(scope="module")
def search_handle():
    """one handle, one slot per case of search_slots(); archives built through alego_lm_add_keyframe from constructed clouds"""
    cases = search_slots()
    h = binding.Handle(_params(False), n_slots=len(cases))
    h.map_enable(257, 1 << 17)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    refs = []
    for s, (name, D, kp, st, mj, md) in enumerate(cases):
        add_frames(h, s, [cloud_of(x) for x in D], poses=kp)
        assert h.map_status(s)[:2] == (len(D), 0), name
        if st is not None and len(st):
            h.map_set_stamps(0, st, slot=s)
        st = h.map_get_stamps(slot=s)
        gap = h.params.lc_min_time_gap
        refs.append(dict(name=name, D=D, kp=kp, st=st, mj=mj, md=md, np=candidates_np(D, kp, st, gap, mj, md, N_CAND),
                         twin=binding.loop_appearance_candidates(D, kp, st, gap, mj, md, N_CAND)))
    yield dict(h=h, refs=refs)
    h.close()


def check_search(r, ref, tag):
    ids, dists, shifts, nel = ref["np"]
    n = len(ref["D"])
    assert r["latest_id"] == n - 1, (tag, r["latest_id"])
    assert (r["n_eligible"], r["n_cand"]) == (nel, len(ids)), (tag, r["n_eligible"], r["n_cand"], nel, len(ids))
    for g, w, t, what in zip((r["cand_id"], r["cand_dist"], r["cand_shift"]), (ids, dists, shifts), ref["twin"], ("ids", "dists", "shifts")):
        assert np.array_equal(g, w) and np.array_equal(t, w), (tag, what, g, w, t)
    assert r["status"] == (1 if len(ids) else 0) and r["closest_id"] == (int(ids[0]) if len(ids) else -1) and r["verified"] == -1, (tag, r)


def run_search(h, refs, slots, same_gates_only=True):
    """the gates are per call: slots are grouped by (max_jump, max_dist); returns {slot: result}"""
    out = {}
    groups = {}
    for s in slots:
        groups.setdefault((refs[s]["mj"], refs[s]["md"]), []).append(s)
    for (mj, md), sl in groups.items():
        for s, r in zip(sl, h.loop_search_appearance(sl, n_cand=N_CAND, verify=0, max_jump=mj, max_dist=md)):
            out[s] = r
    return out


@pytest.mark.gpu
def test_search_is_the_brute_force_over_the_eligible_frames(search_handle):
    h, refs = search_handle["h"], search_handle["refs"]
    n = len(refs)
    # what the cases are there for
    by = {r["name"]: r for r in refs}
    assert by["255 frames, all ineligible"]["np"][3] == 0 and by["256 frames, exactly one eligible"]["np"][0].tolist() == [77]
    assert by["257 frames, n_cand - 1 eligible"]["np"][3] == N_CAND - 1 and sorted(by["257 frames, n_cand - 1 eligible"]["np"][0].tolist()) == [3, 200, 255]
    x = by["257 frames, eligibility not a prefix"]
    el = eligible_np(x["kp"], x["st"], 30.0, 0.0)
    assert 0 < el.sum() < 256 and not el[:el.sum()].all() and x["np"][3] == el.sum()
    x = by["duplicate descriptors"]["np"]
    assert x[0][0] == 0 and (np.diff(x[1]) == 0).any() and (np.diff(x[0])[np.diff(x[1]) == 0] > 0).all()
    assert by["an all-zero newest frame"]["np"][3] == 0
    x = by["max_jump binding"]
    assert 0 < x["np"][3] < 59 and x["np"][3] == eligible_np(x["kp"], x["st"], 30.0, 25.0).sum()
    assert by["max_dist binding"]["np"][0].tolist() == [13, 40] and by["max_dist binding"]["np"][3] == 59
    assert by["n_cand frames"]["np"][3] == N_CAND - 1 and by["2 frames"]["np"][0].tolist() == [0]
    # every slot in one call per pair of gates (the three ungated groups: one call with all of them), pruned
    whole = run_search(h, refs, list(range(n)))
    for s in range(n):
        check_search(whole[s], refs[s], refs[s]["name"])
    ungated = [s for s in range(n) if refs[s]["mj"] == 0 and refs[s]["md"] == 0]
    assert len(ungated) >= 6
    variants = {}
    h.set_option("ALEGO_RL_BRUTE", 1)
    variants["brute"] = run_search(h, refs, list(range(n)))
    h.set_option("ALEGO_RL_BRUTE", 0)
    h.set_option("ALEGO_RL_BUDGET", 1)   # chunks of one query
    variants["chunks of one query"] = run_search(h, refs, list(range(n)))
    h.set_option("ALEGO_RL_BUDGET", 1 << 22)
    variants["reversed"] = run_search(h, refs, list(range(n))[::-1])
    variants["slot by slot"] = {s: run_search(h, refs, [s])[s] for s in range(n)}
    for tag, res in variants.items():
        for s in range(n):
            check_search(res[s], refs[s], f"{refs[s]['name']} ({tag})")
            for k in whole[s]:
                assert_bit_equal(np.asarray(res[s][k]), np.asarray(whole[s][k]), f"{refs[s]['name']} ({tag}): {k}")


ROUND_FRAMES = 8


def round_slots():
    """per slot: (the (corner, surf, outlier) of 8 frames, key poses (8, 6), the frame built to be the best candidate or None).  A few hundred points per
    frame, one per non-zero bin of a random descriptor.  Slot 0: frames without a corner cloud (1, 5 and the newest, 7) and without an outlier cloud
    (2, 5).  Slots 1 and 2: the newest frame's descriptor is frame 0's / frame 6's turned by 11 sectors with one bin in twenty redrawn."""
    rng = np.random.default_rng(23)
    kp = lambda: np.c_[rng.uniform(-30, 30, (ROUND_FRAMES, 3)), rng.uniform(-0.05, 0.05, (ROUND_FRAMES, 2)), rng.uniform(-3, 3, (ROUND_FRAMES, 1))].astype(F32)
    frames = []
    for f, a in enumerate(cloud_of(D) for D in _sparse(rng, ROUND_FRAMES)):
        if f == 5:
            frames.append((EMPTY, a, EMPTY))
        elif f in (1, 7):
            frames.append((EMPTY, a[0::2], a[1::2]))
        elif f == 2:
            frames.append((a[0::2], a[1::2], EMPTY))
        else:
            frames.append(split3(a))
    out = [(frames, kp(), None)]
    for best in (0, ROUND_FRAMES - 2):
        D = _sparse(rng, ROUND_FRAMES)
        q = np.roll(D[best], 11, axis=0)
        redraw = rng.random(q.shape) < 0.05
        q[redraw] = rng.integers(1, 256, int(redraw.sum()))
        D[ROUND_FRAMES - 1] = q
        out.append(([split3(cloud_of(x)) for x in D], kp(), best))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("search_num", [None, 0])
def test_every_round_is_the_attempt_on_its_candidate(search_num):
    """fitness_max = 1e-12 rejects every attempt, so verify = 4 runs all four rounds and the result left behind is round 3's: the guess is candidate 3's and
    the ICP numbers are those of alego_loop_closure_icp on the same frames (the archive's, the newest under guess6) — for frames with an empty corner or
    outlier cloud, for windows clipped at frame 0 and at frame nf - 2, with the default lc_search_num and with 0.  verify = 1: the same for candidate 0."""
    p = _params(False) if search_num is None else _params(False, lc_search_num=search_num)
    sn, nf = p.lc_search_num, ROUND_FRAMES
    assert sn == (25 if search_num is None else 0)
    slots = round_slots()
    stamps = np.arange(nf) * 100.0   # every older frame is eligible
    # the CPU side: numpy alone yields four candidates for every slot, and the shapes are what the docstring of round_slots says
    want = []
    for s, (fr, kp, best) in enumerate(slots):
        desc = np.array([desc_np(np.concatenate(f), MAX_RANGE, Z_OFFSET)[0] for f in fr])
        ids, dists, shifts, nel = candidates_np(desc, kp, stamps, p.lc_min_time_gap, n_cand=N_CAND)
        assert nel == nf - 1 and len(ids) == N_CAND == 4, (s, ids, nel)
        assert best is None or ids[0] == best, (s, ids, dists)
        assert min(sum(len(c) for c in f) for f in fr) >= 200, s
        want.append((ids, dists, shifts))
    n_of = lambda k: [len(f[k]) for f in slots[0][0]]
    assert [i for i, n in enumerate(n_of(0)) if n == 0] == [1, 5, 7] and [i for i, n in enumerate(n_of(2)) if n == 0] == [2, 5] and min(n_of(1)) > 0
    assert (slots[1][2], slots[2][2]) == (0, nf - 2)
    h = binding.Handle(p, n_slots=3)
    h.map_enable(16, 1 << 14)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    for s, (fr, kp, _) in enumerate(slots):
        for f in range(nf):
            h.lm_add_keyframe(kp[f], *fr[f], slot=s)
        assert h.map_status(s)[:2] == (nf, 0), s
        h.map_set_stamps(0, stamps, slot=s)
    arch = [[h.map_get_keyframe(j, slot=s) for j in range(nf)] for s in range(3)]
    for verify, k in ((4, 3), (1, 0)):
        res = h.loop_search_appearance([0, 1, 2], n_cand=4, verify=verify, fitness_max=1e-12)
        assert len(res) == 3
        for s, r in enumerate(res):
            tag = f"lc_search_num {sn}, verify {verify}, slot {s}"
            for g, w, what in zip((r["cand_id"], r["cand_dist"], r["cand_shift"]), want[s], ("ids", "dists", "shifts")):
                assert np.array_equal(g, w), (tag, what, g, w)
            assert (r["n_cand"], r["verified"], r["status"], r["latest_id"]) == (4, -1, 1, nf - 1), (tag, r)
            c = int(r["cand_id"][k])
            assert r["closest_id"] == c, (tag, r["closest_id"], r["cand_id"])
            assert_bit_equal(r["guess6"], guess_of(slots[s][1], c, int(r["cand_shift"][k])), f"{tag}: guess6")
            lo, hi = max(0, c - sn), min(nf - 2, c + sn)
            a = arch[s]
            assert_bit_equal(a[c]["pose"], slots[s][1][c], f"{tag}: the archived pose")
            frames = [(r["guess6"], a[nf - 1]["corner"], a[nf - 1]["surf"], a[nf - 1]["outlier"])] + [(a[j]["pose"], a[j]["corner"], a[j]["surf"], a[j]["outlier"]) for j in range(lo, hi + 1)]
            one, _ = h.loop_closure_icp(frames)
            print(f"{tag}: candidate {c} window [{lo}, {hi}]; search: n_source {r['n_source']} n_target {r['n_target']} converged {r['converged']} iterations {r['iterations']} "
                  f"fitness {r['fitness']:.9g}; single attempt: {one['n_source']} {one['n_target']} {one['converged']} {one['iterations']} {one['fitness']:.9g}; "
                  f"|icp_final - T| {np.abs(r['icp_final'] - one['T']).max():.3g}")
            assert r["n_source"] == sum(len(x) for x in slots[s][0][nf - 1]) and r["n_target"] > 0, (tag, r)
            assert (one["n_source"], one["n_target"], one["converged"]) == (r["n_source"], r["n_target"], r["converged"]), (tag, one, r)
            assert abs(one["iterations"] - r["iterations"]) <= 1, (tag, one, r)
            assert np.abs(r["icp_final"] - one["T"]).max() < 1e-5, (tag, r["icp_final"], one["T"])
            assert abs(one["fitness"] - r["fitness"]) < 1e-6 * max(1.0, r["fitness"]), (tag, one["fitness"], r["fitness"])
    h.close()


def moved_lap_handle(p, starts, steps):
    """replay_handle with the appearance search on and every slot's frames above 30 moved by the ramp; returns (handle, unmoved key poses per slot)"""
    h = replay_handle(p, starts, steps)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    kp0 = []
    for s in range(len(starts)):
        nf, dropped = h.map_status(s)[:2]
        assert dropped == 0 and nf > RAMP_FROM + 2, (s, nf, dropped)
        kp = np.array([h.map_get_keyframe(j, slot=s)["pose"] for j in range(nf)], F32).reshape(-1, 6)
        h.map_set_keyposes(0, ramp(kp), slot=s)
        kp0.append(kp)
    return h, kp0


def check_against_emulation(p, got, dev, kp_unmoved, tag, fitness_max=None, opts=None):
    """one slot's result against numpy (candidates) and the oracle's loop_icp on the device's own archive; returns the emulation's status"""
    kp, st, n = dev["poses"], dev["stamps"], len(dev["poses"])
    desc = dev.setdefault("desc", np.array([desc_np(np.concatenate(dev["frame"](j)), MAX_RANGE, Z_OFFSET)[0] for j in range(n)]))
    o = dict(max_jump=0.0, max_dist=0)
    o.update(opts or {})
    ids, dists, shifts, nel = candidates_np(desc, kp, st, p.lc_min_time_gap, o["max_jump"], o["max_dist"], N_CAND)
    assert got["latest_id"] == n - 1 and got["n_eligible"] == nel and got["n_cand"] == len(ids), (tag, got, nel, ids)
    assert np.array_equal(got["cand_id"], ids) and np.array_equal(got["cand_dist"], dists) and np.array_equal(got["cand_shift"], shifts), (tag, got, ids, dists, shifts)
    if len(ids) == 0:
        assert got["status"] == 0 and got["closest_id"] == -1, (tag, got)
        return 0
    i0, s0 = int(ids[0]), int(shifts[0])
    want, g, t_correct, between = emulate(p, kp, dev["frame"], i0, s0)
    fmax = p.lc_fitness_max if fitness_max is None else fitness_max
    status = 2 if want["converged"] and want["fitness"] <= fmax else 1
    print(f"{tag}: {n} frames, {nel} eligible, frame {i0} D {dists[0]} (next {dists[1] if len(dists) > 1 else '-'}) shift {s0}; oracle: iterations {want['iterations']} fitness {want['fitness']:.4f} "
          f"-> status {status}; device: iterations {got['iterations']} fitness {got['fitness']:.4f} status {got['status']}")
    assert got["closest_id"] == i0, (tag, got["closest_id"], i0)
    assert_bit_equal(got["guess6"], g, f"{tag}: guess6")
    assert (got["status"], got["n_source"], got["n_target"], got["converged"]) == (status, want["n_source"], want["n_target"], want["converged"]), (tag, got, want)
    assert got["verified"] == (0 if status == 2 else -1), (tag, got["verified"])
    assert abs(got["iterations"] - want["iterations"]) <= 1, (tag, got["iterations"], want["iterations"])
    assert np.abs(got["icp_final"] - want["T"]).max() < 1e-5, (tag, got["icp_final"], want["T"])
    assert np.abs(got["t_correct"] - t_correct).max() < 1e-5, (tag, got["t_correct"], t_correct)
    assert np.abs(got["between"] - between).max() < 1e-5, (tag, got["between"], between)
    assert abs(got["fitness"] - want["fitness"]) < 1e-6 * max(1.0, want["fitness"]), (tag, got["fitness"], want["fitness"])
    assert got["noise_variance"] == float(F32(got["fitness"]))
    wc = world_correction_np(got["t_correct"], kp[n - 1])
    assert np.abs(got["T"] - wc).max() < 1e-5 * max(1.0, np.abs(got["t_correct"][:3, 3]).max()), (tag, got["T"], wc)
    return status


LAP_SLOTS = 8


@pytest.fixture(scope="module")
def moved_lap():
    p = _params(False)
    starts = [(s * 37) % LAP for s in range(LAP_SLOTS)]
    h, kp0 = moved_lap_handle(p, starts, 545)
    devs = [device_ref(h, s) for s in range(LAP_SLOTS)]
    radius = h.loop_search(list(range(LAP_SLOTS)))
    res = h.loop_search_appearance(list(range(LAP_SLOTS)))
    yield dict(p=p, h=h, kp0=kp0, devs=devs, radius=radius, res=res)
    h.close()


@pytest.mark.gpu
def test_lap_with_drifted_poses_against_numpy_and_the_oracle(moved_lap):
    O = _O()
    p, h, res = moved_lap["p"], moved_lap["h"], moved_lap["res"]
    good = 0
    for s in range(LAP_SLOTS):
        dev, kp0 = moved_lap["devs"][s], moved_lap["kp0"][s]
        kpd, n = dev["poses"], len(dev["poses"])
        assert_bit_equal(kpd, ramp(kp0), f"slot {s}: the archive holds the moved poses")
        # the radius rule where the drift puts the robot (module docstring): the library's and the oracle's detection find nothing
        at = kpd[n - 1, :3].astype(np.float64)
        assert binding.loop_detect(p, kpd, dev["stamps"], at) == -1 and O.loop_detect(p, kpd, dev["stamps"], at) == -1, s
        assert O.loop_detect(p, kp0, dev["stamps"], kp0[n - 1, :3].astype(np.float64)) >= 0, s
        # alego_loop_search reads the slot's t_map2laser_, which the ramp does not move: it returns what the oracle's detection returns there
        assert moved_lap["radius"][s]["closest_id"] == O.loop_detect(p, kpd, dev["stamps"], dev["cur"]), s
        status = check_against_emulation(p, res[s], dev, kp0, f"slot {s}")
        assert status in (1, 2)
        if status == 2:
            dp, da = pose_gap(res[s]["t_correct"], kp0[n - 1])
            print(f"slot {s}: t_correct {dp:.4f} m {da:.5f} rad from the unmoved newest pose")
            if dp < POS_TOL and da < ANG_TOL:
                good += 1
    assert good >= 1, "no slot was closed at the right place"


@pytest.mark.gpu
def test_search_changes_no_device_state(moved_lap):
    h = moved_lap["h"]
    ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
    snap = lambda s: (h.debug_get("lm_state", slot=s), h.debug_get("lm_info", slot=s), h.map_assemble(ALL, slot=s), h.map_get_stamps(slot=s),
                      np.array([h.map_get_keyframe(j, slot=s)["pose"] for j in range(h.map_status(s)[0])], F32), np.array(h.map_status(s)))
    before = [snap(s) for s in (0, 5)]
    again = h.loop_search_appearance([0, 5])
    after = [snap(s) for s in (0, 5)]
    for b, a in zip(before, after):
        for x, y, what in zip(b, a, ("lm_state", "lm_info", "the archive", "stamps", "key poses", "map_status")):
            assert_bit_equal(x, y, what)
    h.set_option("ALEGO_LC_BUDGET", 1)   # one slot per ICP chunk
    chunked = h.loop_search_appearance([5, 0])
    h.set_option("ALEGO_LC_BUDGET", 1 << 21)
    for s, a, c in ((0, again[0], chunked[1]), (5, again[1], chunked[0])):
        for k in a:
            assert_bit_equal(np.asarray(a[k]), np.asarray(moved_lap["res"][s][k]), f"slot {s} repeated: {k}")
            assert_bit_equal(np.asarray(c[k]), np.asarray(a[k]), f"slot {s} reversed and chunked: {k}")


@pytest.mark.gpu
def test_gates_on_a_slot_without_a_revisit():
    """470 steps: no revisit yet.  On this symmetric synthetic world the best candidate is a frame seen the other way round, which the ICP accepts
    (DESIGN.md section 16): the device reports what the emulation reports, with the gates off and with each gate binding."""
    p = _params(False)
    h, kp0 = moved_lap_handle(p, [37], 470)
    dev = device_ref(h, 0)
    n = len(dev["poses"])
    r = h.loop_search_appearance([0])[0]
    status = check_against_emulation(p, r, dev, kp0[0], "gates off")
    dp, da = pose_gap(r["t_correct"], kp0[0][n - 1])
    print(f"gates off: status {status}, t_correct {dp:.2f} m {da:.4f} rad from the unmoved newest pose")
    assert status == 2, "the aliased frame is accepted by the oracle's ICP with the default threshold"
    cut = r["fitness"] * 0.9
    r1 = h.loop_search_appearance([0], fitness_max=cut)[0]
    assert check_against_emulation(p, r1, dev, kp0[0], "fitness_max below the fitness", fitness_max=cut) == 1
    for k in r:
        if k not in ("status", "verified"):
            assert_bit_equal(np.asarray(r1[k]), np.asarray(r[k]), f"fitness_max changes the verdict alone: {k}")
    jump = float(np.linalg.norm(dev["poses"][r["cand_id"], :3] - dev["poses"][n - 1, :3], axis=1).min())
    r2 = h.loop_search_appearance([0], max_jump=0.5 * jump)[0]
    ids = candidates_np(dev["desc"], dev["poses"], dev["stamps"], p.lc_min_time_gap, 0.5 * jump, 0, N_CAND)
    assert np.array_equal(r2["cand_id"], ids[0]) and r2["n_eligible"] == ids[3]
    if len(ids[0]) == 0:
        assert r2["status"] == 0 and r2["closest_id"] == -1
    assert not set(r2["cand_id"].tolist()) & set(r["cand_id"].tolist())
    tiny = h.loop_search_appearance([0], max_jump=1e-3)[0]
    assert (tiny["status"], tiny["n_eligible"], tiny["n_cand"], tiny["closest_id"]) == (0, 0, 0, -1)
    h.close()


@pytest.mark.gpu
def test_accepted_closures_go_into_the_graph(moved_lap):
    """twin handles replay the same lap with the graph on; the status-2 results go to alego_graph_add_loops unchanged; apply = 1 hands the world
    correction to map -> odom exactly as alego_lm_apply_correction does on the twin"""
    p = moved_lap["p"]
    s_ok = [s for s in range(LAP_SLOTS) if moved_lap["res"][s]["status"] == 2]
    assert s_ok
    start = (s_ok[0] * 37) % LAP
    hs = []
    for _ in range(2):
        h = binding.Handle(p, n_slots=1)
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, _scan(p, k))
        h.replay_assign(0, 0, start)
        h.map_enable(256, 1 << 19)
        h.graph_enable(4)
        h.batch_run(0, 545, stages=7 | binding.REPLAY_BAG, sync=True)
        nf = h.map_status(0)[0]
        kp = np.array([h.map_get_keyframe(j)["pose"] for j in range(nf)], F32).reshape(-1, 6)
        h.map_set_keyposes(0, ramp(kp))
        hs.append(h)
    a, b = hs
    a.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    r = a.loop_search_appearance([0])[0]
    assert r["status"] == 2 and r["closest_id"] == moved_lap["res"][s_ok[0]]["closest_id"], r
    a.graph_add_loops([0], [r])
    e = a.graph_get_edges(kind=1)
    assert e["frm"].tolist() == [r["latest_id"]] and e["to"].tolist() == [r["closest_id"]]
    assert_bit_equal(e["between"][0], r["between"], "the loop edge's measurement")
    assert_bit_equal(e["variance"][0], np.full(6, r["noise_variance"]), "the loop edge's variances")
    g = a.graph_optimize([0], apply=True)[0]
    assert g["status"] == 2 and g["cost"] <= g["cost0"] and g["applied"] == 1 and g["n_loops"] == 1, g
    sb0 = b.debug_get("lm_state")
    b.lm_apply_correction(np.asarray(r["T"], np.float64)[:3, :4].reshape(12), slot=0)
    sa, sb = a.debug_get("lm_state"), b.debug_get("lm_state")
    LD_T_M2O, LD_Q_M2O = 6, 9   # (lm_ctx.h)
    assert_bit_equal(sa[LD_T_M2O:LD_T_M2O + 3], sb[LD_T_M2O:LD_T_M2O + 3], "map -> odom translation")
    assert_bit_equal(sa[LD_Q_M2O:LD_Q_M2O + 4], sb[LD_Q_M2O:LD_Q_M2O + 4], "map -> odom rotation")
    assert np.abs(sb[LD_T_M2O:LD_T_M2O + 3] - sb0[LD_T_M2O:LD_T_M2O + 3]).max() > 1.0, "the correction moved map -> odom"
    a.close()
    b.close()


@pytest.mark.gpu
def test_enabling_changes_no_existing_result():
    """40 scans with and without alego_loop_appearance_enable"""
    p = _params(False)
    runs = []
    for on in (False, True):
        h = binding.Handle(p)
        h.map_enable(64, 1 << 18)
        if on:
            h.loop_appearance_enable()
        poses = []
        for k in range(40):
            flags, odom, mp = h.scan_process(_scan(p, k), stages=7)
            poses.append(np.r_[flags, odom["t"], odom["q"], mp["t"], mp["q"]])
        ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
        runs.append((np.array(poses), h.debug_get("lm_state"), h.debug_get("lm_info"), h.map_assemble(ALL), np.array(h.map_status(0))))
        h.close()
    for x, y, what in zip(runs[0], runs[1], ("poses", "lm_state", "lm_info", "the archive", "map_status")):
        assert_bit_equal(x, y, what)


@pytest.mark.gpu
def test_boundaries():
    p = _params(False)
    h = binding.Handle(p, n_slots=3)
    with pytest.raises(binding.AlegoError):
        h.loop_appearance_enable()            # without the archive
    with pytest.raises(binding.AlegoError):
        h.loop_search_appearance([0])         # not enabled
    h.map_enable(3, 1 << 12)
    with pytest.raises(binding.AlegoError):
        h.loop_search_appearance([0])         # the archive alone is not enough
    h.loop_appearance_enable()
    with pytest.raises(binding.AlegoError):
        h.loop_appearance_enable()            # a second call
    for bad in ([0, 0], [3], [-1]):
        with pytest.raises(binding.AlegoError):
            h.loop_search_appearance(bad)
    with pytest.raises(binding.AlegoError):
        h.loop_search_appearance([0], n_cand=9)
    with pytest.raises(binding.AlegoError):
        h.loop_search_appearance([0], n_cand=2, verify=3)
    assert h.loop_search_appearance([]) == []
    r = h.loop_search_appearance([0, 1, 2])
    assert [x["status"] for x in r] == [0, 0, 0] and [x["latest_id"] for x in r] == [-1, -1, -1] and [x["closest_id"] for x in r] == [-1, -1, -1]
    # a slot whose archive dropped frames is not searchable
    rng = np.random.default_rng(3)
    add_frames(h, 1, [cloud_of(D) for D in _sparse(rng, 5)])
    assert h.map_status(1)[1] > 0
    r = h.loop_search_appearance([0, 1])
    assert [x["status"] for x in r] == [0, -1]
    # NULL info is allowed
    out = (binding.LoopResult * 1)()
    sl = np.array([1], np.int32)
    assert binding.lib().alego_loop_search_appearance(h._h, sl.ctypes.data, 1, None, out, None) == 0 and out[0].status == -1
    h.close()
    # a localising handle
    f = (np.zeros(6, F32), EMPTY, EMPTY, EMPTY)
    h = binding.Handle(p)
    h.loc_enable([f], 0.0)
    with pytest.raises(binding.AlegoError):
        h.loop_appearance_enable()
    h.close()


@pytest.mark.gpu
def test_replay_appearance_agrees_with_the_binding():
    """lc_search_radius 1 m leaves the revisits of the lap to the appearance search, so the hand-over and the " appearance D S" suffix are exercised"""
    import subprocess
    n, every, radius = 556, 50, 1.0
    exe = os.path.join(ROOT, "examples", "replay")
    out = subprocess.run([exe, str(n), "--loop-search", str(every), "--appearance", "--loop-radius", str(radius)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("loop:")]
    p = synth.default_params(16, 1800)
    p.lc_search_radius = radius
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    h.loop_appearance_enable()
    want, by_appearance = [], 0
    for k in range(n):
        h.scan_process(_scan(p, k), stages=7, stamp=0.1 * k)
        if (k + 1) % every == 0:
            r = h.loop_search([0])[0]
            tail = ""
            if r["status"] == 0:
                r = h.loop_search_appearance([0])[0]
                if r["status"] == 2:
                    tail = f" appearance {r['cand_dist'][r['verified']]} {r['cand_shift'][r['verified']]}"
                    by_appearance += 1
            if r["status"] == 2:
                want.append(f"loop: scan {k} slot 0 latest {r['latest_id']} closest {r['closest_id']} fitness {r['fitness']:.9g}{tail}")
    h.close()
    print("\n".join(got))
    assert got == want, (got, want)
    assert by_appearance >= 1 and any(" appearance " in ln for ln in got), got
