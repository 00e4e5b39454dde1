"""Batched loop-closure search over the device key-frame archive (alego_loop_search, kernels_loop.hip), the archive's key-frame
stamps (alego_map_get_stamps / alego_map_set_stamps), the host constraint (alego_loop_constraint) and the grid 1-NN on its own
(alego_debug_nn1).  References come from the oracle's existing functions: Oracle replays give the key-frame ids and stamps,
loop_detect and loop_icp judge each slot's attempt on that slot's archive."""
import os
import re

import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_map_get_stamps", "alego_map_set_stamps", "alego_loop_search", "alego_loop_constraint", "alego_debug_nn1"]
LAP = 560          # the synthetic lap, one HBM bag
F32 = np.float32


def _O():
    from oracle import oracle_py
    return oracle_py


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_loop_search_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in binding.EXPORTS, s


def _initial_guess(pose):
    """:680-687 in f32: AngleAxisf(yaw, Z) * AngleAxisf(pitch, Y) * AngleAxisf(roll, X), toRotationMatrix(), translation = xyz"""
    h = [F32(0.5) * F32(pose[5]), F32(0.5) * F32(pose[4]), F32(0.5) * F32(pose[3])]
    qz = [np.cos(h[0]), F32(0), F32(0), np.sin(h[0])]
    qy = [np.cos(h[1]), F32(0), np.sin(h[1]), F32(0)]
    qx = [np.cos(h[2]), np.sin(h[2]), F32(0), F32(0)]

    def mul(a, b):
        return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]
    w, x, y, z = mul(mul(qz, qy), qx)
    two = F32(2)
    tx, ty, tz = two * x, two * y, two * z
    one = F32(1)
    G = np.zeros((4, 4), F32)
    G[0] = [one - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w, pose[0]]
    G[1] = [ty * x + tz * w, one - (tx * x + tz * z), tz * y - tx * w, pose[1]]
    G[2] = [tz * x - ty * w, tz * y + tx * w, one - (tx * x + ty * y), pose[2]]
    G[3] = [0, 0, 0, 1]
    return G


def _eigen_quaternion_f32(M):
    """Eigen's Quaternionf(Matrix3f) -> (w, x, y, z), f32"""
    M = M.astype(F32)
    t = M[0, 0] + M[1, 1] + M[2, 2]
    q = [F32(0)] * 4
    if t > 0:
        t = np.sqrt(t + F32(1)); q[0] = F32(0.5) * t; t = F32(0.5) / t
        q[1] = (M[2, 1] - M[1, 2]) * t; q[2] = (M[0, 2] - M[2, 0]) * t; q[3] = (M[1, 0] - M[0, 1]) * t
    else:
        i = 0
        if M[1, 1] > M[0, 0]:
            i = 1
        if M[2, 2] > M[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(M[i, i] - M[j, j] - M[k, k] + F32(1))
        q[1 + i] = F32(0.5) * t; t = F32(0.5) / t
        q[0] = (M[k, j] - M[j, k]) * t; q[1 + j] = (M[j, i] + M[i, j]) * t; q[1 + k] = (M[k, i] + M[i, k]) * t
    return [float(v) for v in q]


def constraint_reference(correction, latest, closest):
    """:714-730 restated: t_correct = correction * initial_guess (Matrix4f); pose_from = Pose3(Rot3::Quaternion(Quaternionf(t_correct)),
    t_correct translation); pose_to = Pose3(Rot3::RzRyRx(roll, pitch, yaw), xyz) of the closest key pose; between = from^-1 * to"""
    C4 = np.asarray(correction, F32).reshape(4, 4)
    G = _initial_guess(np.asarray(latest, F32))
    T = np.zeros((4, 4), F32)
    for r in range(4):
        for c in range(4):
            acc = F32(0)
            for k in range(4):
                acc = F32(acc + C4[r, k] * G[k, c])
            T[r, c] = acc
    w, x, y, z = _eigen_quaternion_f32(T[:3, :3])
    Rf = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    tf = T[:3, 3].astype(np.float64)
    r, p, yw = (float(v) for v in np.asarray(closest, F32)[3:6])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(yw), -np.sin(yw), 0], [np.sin(yw), np.cos(yw), 0], [0, 0, 1]])
    Rt = Rz @ Ry @ Rx
    tt = np.asarray(closest, F32)[:3].astype(np.float64)
    B = np.zeros((3, 4))
    B[:, :3] = Rf.T @ Rt
    B[:, 3] = Rf.T @ (tt - tf)
    return T, B


def _rot(axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


@pytest.mark.parametrize("kind", ["random", "near_180"])
def test_loop_constraint_matches_restatement(kind):
    rng = np.random.default_rng(11 if kind == "random" else 12)
    for trial in range(200):
        latest = np.concatenate([rng.uniform(-30, 30, 3), rng.uniform(-np.pi, np.pi, 3)]).astype(F32)
        closest = np.concatenate([rng.uniform(-30, 30, 3), rng.uniform(-np.pi, np.pi, 3)]).astype(F32)
        corr = np.eye(4)
        if kind == "random":
            corr[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0, 0.5))
        else:   # t_correct's rotation near 180 degrees: Eigen's largest-diagonal branch
            G = _initial_guess(latest).astype(np.float64)
            want = _rot(rng.normal(size=3), np.pi - rng.uniform(0, 1e-3))
            corr[:3, :3] = want @ G[:3, :3].T
        corr[:3, 3] = rng.uniform(-2, 2, 3)
        corr = corr.astype(F32)
        t_got, b_got = binding.loop_constraint(corr, latest, closest)
        t_want, b_want = constraint_reference(corr, latest, closest)
        assert np.abs(t_got - t_want).max() <= 1e-6 * max(1.0, np.abs(t_want).max()), (trial, t_got, t_want)
        assert np.abs(b_got - b_want).max() <= 1e-6 * max(1.0, np.abs(b_want).max()), (trial, b_got, b_want)
        if kind == "near_180":
            assert np.trace(t_want[:3, :3]) < -0.9


# ---- GPU: batch replay against the oracle ---------------------------------------------------------------------------
_SCANS = {}


def _scan(p, k):
    if k not in _SCANS:
        _SCANS[k] = synth.scan(p, k)
    return _SCANS[k]


def _params(standalone, **kw):
    p = synth.default_params(16, 1800)
    if standalone:   # the literals of src/LM.cpp:175,210,212 instead of the nodelet's
        p.lc_leaf, p.lc_search_radius, p.lc_fitness_max = 0.4, 10.0, 0.3
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def replay_handle(p, starts, steps, max_frames=256, max_points=1 << 19):
    h = binding.Handle(p, n_slots=len(starts))
    h.replay_create(1, LAP)
    for k in range(LAP):
        h.replay_load(0, k, _scan(p, k))
    for s, st in enumerate(starts):
        h.replay_assign(s, 0, st)
    h.map_enable(max_frames, max_points)
    h.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=False)   # no host call between the steps
    h.synchronize()
    return h


def oracle_replay(p, start, steps, stamp_of=None):
    """the oracle on the same scan sequence; every key frame's stamp: stamp_of(i) of the scan i that saved it (default: the batch rule,
    (mapping frames so far - 1) * scan_period = (i - 1) * scan_period: scan 0 initialises the odometry)"""
    O = _O()
    o = O.Oracle(p)
    stamps = []
    for i in range(steps):
        o.process_scan(_scan(p, (start + i) % LAP))
        n = o.get("lm_keyposes").size // 6
        while len(stamps) < n:
            stamps.append(stamp_of(i) if stamp_of else (i - 1) * p.scan_period)
    poses = o.get("lm_keyposes").reshape(-1, 6).copy()
    return dict(o=o, poses=poses, stamps=np.array(stamps, np.float64), cur=o.get("map_pose")[:3].copy())


def device_ref(h, slot):
    """what the oracle's detectLoopClosure / performLoopClosure see, taken from the device: the archived key frames, key poses and stamps
    and the current map pose.  (Free-running trajectories of the device and the oracle drift apart by up to ~1e-3 m over 400 scans, so
    the oracle judges the search on the slot's own archive; oracle_replay checks the key-frame ids and stamps themselves.)"""
    nf = h.map_status(slot)[0]
    kfs = [h.map_get_keyframe(j, slot=slot) for j in range(nf)]
    poses = np.array([k["pose"] for k in kfs], F32).reshape(-1, 6)
    _, _, m = h.batch_get_pose(slot)
    return dict(poses=poses, stamps=h.map_get_stamps(slot=slot), cur=np.array(m["t"], np.float64),
                frame=lambda j: (kfs[j]["corner"], kfs[j]["surf"], kfs[j]["outlier"]))


def oracle_attempt(p, ref):
    """performLoopClosure (the oracle's loop_detect + loop_icp) on ref's key frames: (closest, icp result or None)"""
    O = _O()
    poses, n = ref["poses"], len(ref["poses"])
    if n == 0:
        return -1, None
    closest = O.loop_detect(p, poses, ref["stamps"], ref["cur"])
    if closest < 0:
        return closest, None
    frames = [(poses[n - 1],) + tuple(ref["frame"](n - 1))]
    for j in range(closest - p.lc_search_num, closest + p.lc_search_num + 1):
        if 0 <= j < n - 1:
            frames.append((poses[j],) + tuple(ref["frame"](j)))
    want, _ = O.loop_icp(p, frames)
    return closest, want


def check_result(p, got, ref, tag):
    """one slot's alego_loop_search result against the oracle; returns the status"""
    poses, n = ref["poses"], len(ref["poses"])
    closest, want = oracle_attempt(p, ref)
    assert got["latest_id"] == n - 1, (tag, got["latest_id"], n)
    assert got["closest_id"] == closest, (tag, got["closest_id"], closest)
    if want is None:
        assert got["status"] == 0, (tag, got)
        return 0
    status = 2 if want["converged"] and want["fitness"] <= p.lc_fitness_max else 1
    assert (got["status"], got["n_source"], got["n_target"], got["converged"]) == (status, want["n_source"], want["n_target"], want["converged"]), (tag, got, want)
    if want["n_target"] == 0:
        return status
    assert abs(got["iterations"] - want["iterations"]) <= 1, (tag, got["iterations"], want["iterations"])
    assert np.abs(got["T"] - want["T"]).max() < 1e-5, (tag, got["T"], want["T"])
    assert abs(got["fitness"] - want["fitness"]) < 1e-6 * max(1.0, want["fitness"]), (tag, got["fitness"], want["fitness"])
    t_want, b_want = binding.loop_constraint(want["T"], poses[n - 1], poses[closest])
    assert np.abs(got["t_correct"] - t_want).max() < 1e-5, (tag, got["t_correct"], t_want)
    assert np.abs(got["between"] - b_want).max() < 1e-5, (tag, got["between"], b_want)
    assert got["noise_variance"] == float(F32(got["fitness"]))
    return status


N_SLOTS = 128                      # two stream groups of 64
START = lambda s: (s * 37) % LAP   # varied start scans


@pytest.fixture(scope="module", params=["nodelet", "standalone"])
def lap(request):
    standalone = request.param == "standalone"
    p = _params(standalone)
    steps = 545 if standalone else 420   # (a 10 m radius only finds the start of the lap once the lap is almost closed)
    h = replay_handle(p, [START(s) for s in range(N_SLOTS)], steps)
    groups, per = h.stream_groups()
    assert groups >= 2
    sample = sorted({s for g in range(groups) for s in (g * per, min(N_SLOTS, (g + 1) * per) - 1)} | {37, 90})
    res = h.loop_search(list(range(N_SLOTS)))
    refs = {s: oracle_replay(p, START(s), steps) for s in sample}   # (one at a time: oracle instances share scratch)
    yield dict(p=p, h=h, steps=steps, res=res, refs=refs, sample=sample, standalone=standalone)
    h.close()


@pytest.mark.gpu
def test_batch_search_matches_oracle(lap):
    p, h, res, refs = lap["p"], lap["h"], lap["res"], lap["refs"]
    statuses = {}
    for s in lap["sample"]:
        ref = refs[s]
        dev = device_ref(h, s)
        st = dev["stamps"]
        # the batch rule: (mapping frames so far - 1) * scan_period.  Key frames are saved on the same scans as in the oracle until the
        # free-running trajectories have drifted apart enough to move a key-frame decision (late in a 545-scan run): the first 300 scans
        n = min(len(st), len(ref["stamps"]))
        agree = int(np.count_nonzero(ref["stamps"][:n] < 300 * p.scan_period))
        assert agree >= 10, (s, agree)
        assert_bit_equal(st[:agree], ref["stamps"][:agree], f"slot {s}: archived stamps")
        assert_bit_equal(np.round(st / p.scan_period) * p.scan_period, st, f"slot {s}: stamps are ordinal * scan_period")
        assert (np.diff(st) > 0).all()
        statuses[s] = check_result(p, res[s], dev, f"slot {s}")
    assert 2 in statuses.values(), statuses
    if not lap["standalone"]:   # the start area is revisited with history frames below closest - lc_search_num < 0
        assert any(res[s]["status"] > 0 and res[s]["closest_id"] < p.lc_search_num for s in lap["sample"])
    assert all(r["status"] >= 0 for r in res)


@pytest.mark.gpu
def test_batch_search_is_independent_of_the_other_slots(lap):
    h, res = lap["h"], lap["res"]
    again = h.loop_search(list(range(N_SLOTS)))
    rev = h.loop_search(list(range(N_SLOTS))[::-1])[::-1]
    for s in (0, 1, 63, 64, 127):
        one = h.loop_search([s])[0]
        for r, tag in ((again[s], "repeated call"), (rev[s], "reversed list"), (one, "alone")):
            for k in res[s]:
                assert_bit_equal(np.asarray(r[k]), np.asarray(res[s][k]), f"slot {s} {tag}: {k}")
    h.set_option("ALEGO_LC_BUDGET", 20000)   # chunks of a slot or two: chunking changes nothing
    small = h.loop_search(list(range(N_SLOTS)))
    h.set_option("ALEGO_LC_BUDGET", 1 << 21)
    for s in range(N_SLOTS):
        for k in res[s]:
            assert_bit_equal(np.asarray(small[s][k]), np.asarray(res[s][k]), f"slot {s} chunked: {k}")


@pytest.mark.gpu
def test_batch_search_equals_single_attempt_icp(lap):
    p, h, res = lap["p"], lap["h"], lap["res"]
    checked = 0
    for s in lap["sample"]:
        r = res[s]
        if r["status"] <= 0:
            continue
        lo, hi = max(0, r["closest_id"] - p.lc_search_num), min(r["latest_id"] - 1, r["closest_id"] + p.lc_search_num)
        frames = []
        for j in [r["latest_id"]] + list(range(lo, hi + 1)):
            k = h.map_get_keyframe(j, slot=s)
            frames.append((k["pose"], k["corner"], k["surf"], k["outlier"]))
        one, _ = h.loop_closure_icp(frames)
        assert (one["n_target"], one["converged"], one["n_source"]) == (r["n_target"], r["converged"], r["n_source"]), (s, one, r)
        assert abs(one["iterations"] - r["iterations"]) <= 1
        assert np.abs(one["T"] - r["T"]).max() < 1e-5
        assert abs(one["fitness"] - r["fitness"]) < 1e-6 * max(1.0, r["fitness"])
        checked += 1
    assert checked >= 1


@pytest.mark.gpu
def test_rejected_and_too_few_correspondences():
    """Same slots, other thresholds: lc_fitness_max tiny -> attempted and rejected (the rest bit-identical to the default handle's
    result for the same start); icp_max_corr_dist tiny -> fewer than 3 correspondences, converged = 0.  Both against the oracle."""
    steps, start = 420, START(0)
    base = replay_handle(_params(False), [start], steps)
    want = base.loop_search([0])[0]
    base.close()
    assert want["status"] == 2, want
    for kw, conv in ((dict(lc_fitness_max=1e-9), 1), (dict(icp_max_corr_dist=1e-4), 0)):
        p = _params(False, **kw)
        h = replay_handle(p, [start], steps)
        got = h.loop_search([0])[0]
        assert got["status"] == 1 and got["converged"] == conv, (kw, got)
        if conv:
            for k in want:
                if k != "status":
                    assert_bit_equal(np.asarray(got[k]), np.asarray(want[k]), f"{kw}: {k}")
        else:
            assert got["iterations"] == 0
        check_result(p, got, device_ref(h, 0), str(kw))
        h.close()


@pytest.mark.gpu
def test_search_leaves_device_state_untouched():
    p = _params(False)
    starts, steps = [0, 280], 420
    ha, hb = replay_handle(p, starts, steps), replay_handle(p, starts, steps)
    r = ha.loop_search([0, 1, 0])
    assert r[0]["status"] > 0
    for x in (ha, hb):
        x.batch_run(steps, 20, stages=7 | binding.REPLAY_BAG, sync=True)
    ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
    for s in range(2):
        fa, oa, ma = ha.batch_get_pose(s)
        fb, ob, mb = hb.batch_get_pose(s)
        for k in ("t", "q", "params"):
            assert_bit_equal(oa[k], ob[k], f"slot {s} odometry {k}")
            assert_bit_equal(ma[k], mb[k], f"slot {s} map {k}")
        assert ha.map_status(s) == hb.map_status(s)
        assert_bit_equal(ha.map_assemble(ALL, slot=s), hb.map_assemble(ALL, slot=s), f"slot {s} global map")
        assert_bit_equal(ha.map_get_stamps(slot=s), hb.map_get_stamps(slot=s), f"slot {s} stamps")
    ha.close(); hb.close()


@pytest.mark.gpu
def test_stamped_path_and_set_stamps():
    """alego_scan_process with jittered stamps: every key frame carries the stamp of the scan that saved it; the spatially nearest
    candidates are too recent, so the stamps decide; alego_map_set_stamps moves the choice exactly as loop_detect predicts."""
    O = _O()
    p = _params(False)
    steps = 420
    rng = np.random.default_rng(5)
    stamps = 1000.0 + np.cumsum(rng.uniform(0.05, 0.15, steps))
    h = binding.Handle(p)
    h.map_enable(256, 1 << 19)
    for i in range(steps):
        h.scan_process(_scan(p, i), stages=7, stamp=float(stamps[i]))
    assert_bit_equal(h.map_get_stamps(), oracle_replay(p, 0, steps, stamp_of=lambda i: float(stamps[i]))["stamps"], "archived stamps")
    ref = device_ref(h, 0)
    poses, n = ref["poses"], len(ref["poses"])
    d2 = ((poses[:, :3] - ref["cur"].astype(F32)) ** 2).sum(1)
    got = h.loop_search([0])[0]
    assert check_result(p, got, ref, "stamped") > 0
    assert int(np.argmin(d2)) != got["closest_id"], "the nearest key pose should be too recent"
    # make the chosen frame (and its neighbours) recent: the next one old enough wins
    st = ref["stamps"].copy()
    c = got["closest_id"]
    st[c] = st[-1] - 1.0
    h.map_set_stamps(c, st[c:c + 1])
    assert_bit_equal(h.map_get_stamps(), st, "stamps after alego_map_set_stamps")
    ref2 = dict(ref, stamps=st)
    want2 = O.loop_detect(p, poses, st, ref["cur"])
    got2 = h.loop_search([0])[0]
    assert want2 != c and got2["closest_id"] == want2, (c, want2, got2["closest_id"])
    check_result(p, got2, ref2, "after set_stamps")
    h.close()


# ---- GPU: the grid 1-NN on its own ----------------------------------------------------------------------------------
def _brute(tgt, q):
    """f32 ((dx dx + dy dy) + dz dz), lowest index on ties; (-1, FLT_MAX) when nothing is below FLT_MAX"""
    idx = np.full(len(q), -1, np.int32)
    best = np.full(len(q), np.finfo(F32).max, F32)
    if len(tgt) == 0:
        return idx, best
    T = tgt[:, :3].astype(F32)
    for b in range(0, len(q), 256):
        Q = q[b:b + 256, :3].astype(F32)
        with np.errstate(over="ignore", invalid="ignore"):
            dx = T[None, :, 0] - Q[:, None, 0]
            dy = T[None, :, 1] - Q[:, None, 1]
            dz = T[None, :, 2] - Q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
        d = np.where(np.isnan(d), np.inf, d)
        a = np.argmin(d, axis=1)
        m = d[np.arange(len(Q)), a]
        ok = m < np.finfo(F32).max
        idx[b:b + 256] = np.where(ok, a, -1)
        best[b:b + 256] = np.where(ok, m, np.finfo(F32).max)
    return idx, best


def _pts(xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    return np.concatenate([xyz, np.zeros((len(xyz), 1), F32)], axis=1)


def _nn_case(name):
    rng = np.random.default_rng(100 + NN_CASES.index(name))
    if name == "ties_duplicates":
        lat = rng.integers(-4, 5, (3000, 3)).astype(F32)
        tgt = np.concatenate([lat, lat[:500]])              # exact duplicates at higher indices
        q = np.concatenate([lat[:300], lat[:300] + 0.5, rng.integers(-5, 6, (300, 3)) + 0.5])
    elif name == "cell_and_binade_boundaries":
        base = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, -1.0, -2.0, -0.5], F32)
        vals = np.concatenate([base, np.nextafter(base, F32(np.inf)), np.nextafter(base, F32(-np.inf))])
        tgt = rng.choice(vals, (4000, 3))
        q = np.concatenate([rng.choice(vals, (1000, 3)), rng.choice(vals, (1000, 3)) + rng.normal(0, 1e-6, (1000, 3)).astype(F32)])
    elif name == "far_queries":
        tgt = rng.uniform(-20, 20, (5000, 3))
        dirs = rng.normal(size=(1000, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        q = dirs * rng.uniform(120, 5000, (1000, 1))
    elif name == "one_cell":
        tgt = np.full((3000, 3), 7.25, F32) + rng.integers(0, 2, (3000, 3)).astype(F32) * F32(1e-6)
        q = np.concatenate([tgt[:500], rng.uniform(-10, 20, (500, 3))])
    elif name == "one_point":
        tgt = np.array([[1.5, -2.0, 0.25]], F32)
        q = rng.uniform(-300, 300, (1000, 3))
    elif name == "large_uniform":
        tgt = rng.uniform(-60, 60, (100000, 3)) * [1, 1, 0.1]
        q = rng.uniform(-80, 80, (2000, 3)) * [1, 1, 0.2]
    elif name == "large_clustered":
        c = rng.uniform(-50, 50, (40, 3))
        tgt = c[rng.integers(0, 40, 100000)] + rng.normal(0, 0.3, (100000, 3))
        q = np.concatenate([c[rng.integers(0, 40, 1500)] + rng.normal(0, 1.0, (1500, 3)), rng.uniform(-200, 200, (500, 3))])
    elif name == "empty_and_nonfinite":
        tgt = rng.uniform(-5, 5, (100, 3))
        q = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [1, 1, 1]], np.float64)
    return _pts(tgt), _pts(q)


NN_CASES = ["ties_duplicates", "cell_and_binade_boundaries", "far_queries", "one_cell", "one_point", "large_uniform", "large_clustered",
            "empty_and_nonfinite"]


@pytest.fixture(scope="module")
def nn_handle():
    h = binding.Handle(synth.default_params(16, 1800))
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NN_CASES)
def test_debug_nn1_is_exact(nn_handle, name):
    tgt, q = _nn_case(name)
    gi, gd = nn_handle.debug_nn1(tgt, q)
    wi, wd = _brute(tgt, q)
    assert_bit_equal(gi, wi, f"{name}: indices")
    assert_bit_equal(gd, wd, f"{name}: squared distances")
    if name == "empty_and_nonfinite":
        ei, ed = nn_handle.debug_nn1(np.zeros((0, 4), F32), q)
        assert (ei == -1).all() and (ed == np.finfo(F32).max).all()


# ---- GPU: edge cases --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_edge_cases():
    p = _params(False)
    L = binding.lib()
    h = binding.Handle(p, n_slots=2)
    out = (binding.LoopResult * 1)()
    sl = np.zeros(1, np.int32)
    assert L.alego_loop_search(h._h, sl.ctypes.data, 1, out) == binding.ERR_ARG, "archive off"
    h.map_enable(16, 1000)
    bad = np.array([2], np.int32)
    assert L.alego_loop_search(h._h, bad.ctypes.data, 1, out) == binding.ERR_ARG, "slot out of range"
    r = h.loop_search([0, 1])
    assert [x["status"] for x in r] == [0, 0] and r[0]["latest_id"] == -1 and r[0]["closest_id"] == -1, "no key frames: no candidate"
    assert h.loop_search([]) == []
    h.close()
    # an archive that dropped frames: the newest key frame is missing, the slot is not searchable
    hd = replay_handle(p, [0], 60, max_frames=3, max_points=1 << 16)
    assert hd.map_status(0)[1] > 0
    assert hd.loop_search([0])[0]["status"] < 0
    hd.close()
