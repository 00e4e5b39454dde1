"""A slot's archive of a mapping handle handed to a localising handle on the device (alego_loc_enable_from_map / alego_loc_update_from_map,
kernels_loc.hip loc_fill).

The reference is the host route of the same build: the frames pulled with alego_map_get_keyframe and handed to alego_loc_enable, whose
sequential build is untouched.  Everything is compared bit for bit: the store rows (debug read-outs "ls_*"), lm_keyposes, alego_loc_status,
and what the scans after it produce.  Constructed archives are filled with alego_lm_add_keyframe on an archive-enabled handle (no SLAM run).
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alego_amd import binding
from util import assert_bit_equal, quat_angle
from test_localize import EMPTY, F32, LD_LOC_P, LD_M2O, LI_RUN, _WindowAsKeyFrames, _euler_zyx, _params, _rc, _scan, emulate, select_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_loc_enable_from_map", "alego_loc_update_from_map"]
K, RADIUS = 10, 6.0
STATE = ("lm_state", "lm_window", "lm_corner_map_ds", "lm_surf_map_ds")


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_handover_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _guards_clean():
    bad, rep = binding.check_guards()
    assert bad <= 0, rep   # (-1: the guards are off in this run)


def _tuples(frames):
    return [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames]


def _mapping_handle(frames, max_frames=64, max_points=1 << 20, n_slots=1, slot=0):
    """an archive-enabled handle whose slot holds `frames` (dicts or tuples), inserted with alego_lm_add_keyframe"""
    h = binding.Handle(_params(), n_slots=n_slots)
    h.map_enable(max_frames, max_points)
    for f in frames:
        t = (f["pose"], f["corner"], f["surf"], f["outlier"]) if isinstance(f, dict) else f
        h.lm_add_keyframe(*t, slot=slot)
    assert h.map_status(slot)[:2] == (len(frames), 0)
    return h


def _pull(hm, slot=0):
    return [hm.map_get_keyframe(i, slot=slot) for i in range(hm.map_status(slot)[0])]


def _assert_store_equal(a, b, n, tag):
    assert a.loc_status()["frames"] == b.loc_status()["frames"] == n, (tag, a.loc_status(), b.loc_status())
    for f in range(n):
        x, y = a.loc_store_frame(f), b.loc_store_frame(f)
        for name in x:
            assert_bit_equal(x[name], y[name], f"{tag} frame {f} {name}")
    assert_bit_equal(a.debug_get("lm_keyposes"), b.debug_get("lm_keyposes"), f"{tag} lm_keyposes")
    assert a.loc_status() == b.loc_status(), (tag, a.loc_status(), b.loc_status())


def _assert_state_equal(a, b, tag, rebuilds_ahead=0, sa=0, sb=0):
    """a's slot sa against b's slot sb; rebuilds_ahead: local-map rebuilds a has done more than b"""
    for name in STATE:
        assert_bit_equal(a.debug_get(name, slot=sa), b.debug_get(name, slot=sb), f"{tag} {name}")
    x, y = a.loc_status(sa), b.loc_status(sb)
    assert x["rebuilds"] - rebuilds_ahead == y["rebuilds"], (tag, x, y)
    assert {k: v for k, v in x.items() if k != "rebuilds"} == {k: v for k, v in y.items() if k != "rebuilds"}, (tag, x, y)


def _place(h, pose7, slot=0):
    h.lm_apply_correction(_rc(pose7[:3], pose7[3:]), slot=slot)
    h.set_lm_params(np.r_[pose7[:3], _euler_zyx(pose7[3:])], slot=slot)


def _refused(fn, code, text=None):
    with pytest.raises(binding.AlegoError) as ei:
        fn()
    assert f"({code})" in str(ei.value), ei.value
    if text:
        assert text in str(ei.value), ei.value


# ---- 1. the store equals the host route, on constructed archives ----------------------------------------------------------------
CAP_C, CAP_S, CAP_O = 20 * 6 * 16, 28800 // 2, 28800 // 4   # key-frame capacities of a 16 x 1800 handle (lm_host_create)
CHUNK = 4
TYPES = ["empty", "one", "caps", "t8191", "t8192", "t8193", "far"]
# position of type t in arrangement r of a 9-frame archive; with chunks of 4 the positions 0 4 8 are first, 3 7 last, the others in the middle
ARRANGE = [[0, 1, 2, 3, 4, 5, 7], [3, 7, 0, 1, 2, 4, 5], [1, 0, 3, 4, 7, 2, 8], [2, 4, 5, 0, 1, 3, 6]]


def _cloud(rng, n, half=20.0):
    return np.c_[rng.uniform(-half, half, (n, 2)), rng.uniform(-2, 6, n), rng.uniform(0, 100, n)].astype(F32)


def _typed_frame(kind, rng):
    pose = np.r_[rng.uniform(-5, 5, 3), rng.uniform(-0.3, 0.3, 3)].astype(F32)
    if kind == "empty":
        return (pose, EMPTY, EMPTY, EMPTY)
    if kind == "one":
        return (pose, _cloud(rng, 1), EMPTY, EMPTY)
    if kind == "caps":
        return (pose, _cloud(rng, CAP_C), _cloud(rng, CAP_S), _cloud(rng, CAP_O))
    if kind in ("t8191", "t8192", "t8193"):   # surf + outlier on either side of the vox_small / vox_big boundary
        tot = int(kind[1:])
        return (pose, _cloud(rng, 300), _cloud(rng, tot - 1000), _cloud(rng, 1000))
    if kind == "far":   # beyond PCL's INT_MAX rule at both leaf sizes: stored unsorted
        far = np.array([[0, 0, 0, 1], [1e4, 1e4, 1e4, 2]], F32)
        return (pose, far, np.r_[far[::-1], _cloud(rng, 50)], _cloud(rng, 20))
    return (pose, _cloud(rng, 700), _cloud(rng, 2500), _cloud(rng, 900))   # filler


def _arrangement(r):
    rng = np.random.default_rng(100 + r)
    frames = [None] * 9
    for t, pos in zip(TYPES, ARRANGE[r]):
        frames[pos] = _typed_frame(t, rng)
    return [f if f is not None else _typed_frame("filler", rng) for f in frames]


def test_arrangements_put_every_case_first_middle_and_last_in_a_chunk():
    cls = lambda p: "first" if p % CHUNK == 0 else ("last" if p % CHUNK == CHUNK - 1 else "middle")
    for t in range(len(TYPES)):
        assert {cls(a[t]) for a in ARRANGE} == {"first", "middle", "last"}, TYPES[t]
    for a in ARRANGE:
        assert len(set(a)) == len(a) and max(a) < 9


HANDOVER_CASES = [(0, n, CHUNK, 0) for n in (0, 1, 3, 4, 5, 9)] + [(r, 9, CHUNK, 0) for r in (1, 2, 3)] + [(0, 9, 0, 0), (0, 9, CHUNK, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("arr,n,chunk,extra", HANDOVER_CASES)
def test_store_equals_the_host_route(arr, n, chunk, extra):
    frames = _arrangement(arr)[:n]
    hm = _mapping_handle(frames)
    if n:   # some poses are rewritten behind the archive's back before the hand-over
        rng = np.random.default_rng(n)
        first = n // 2
        hm.map_set_keyposes(first, np.c_[rng.uniform(-8, 8, (n - first, 3)), rng.uniform(-0.5, 0.5, (n - first, 3))].astype(F32))
    a, b = binding.Handle(_params(K)), binding.Handle(_params(K))
    if chunk:
        a.set_option("ALEGO_LOC_CHUNK", chunk)
    a.loc_enable_from_map(hm, 0, RADIUS, capacity=n + extra if extra else 0)
    pulled = _pull(hm)
    assert len(pulled) == n
    b.loc_enable(_tuples(pulled), RADIUS)
    _assert_store_equal(a, b, n, f"arrangement {arr} n {n} chunk {chunk} extra {extra}")
    for f, (pose, c, s, o) in enumerate(frames):   # and the read-outs are what went in
        x = a.loc_store_frame(f)
        assert x["counts"].tolist() == [len(c), len(s) + len(o), len(c), len(s), len(o)], (f, x["counts"])
        assert_bit_equal(x["raw_c"], c, f"frame {f} raw corner")
        assert_bit_equal(x["raw_s"], s, f"frame {f} raw surf")
        assert_bit_equal(x["raw_o"], o, f"frame {f} raw outlier")
        assert_bit_equal(x["pose"][:6], pulled[f]["pose"], f"frame {f} pose")
    for h in (a, b, hm):
        h.close()
    _guards_clean()


# ---- 2. behaviour equals the host route on the lap --------------------------------------------------------------------------------
N_MAP, N_LOC = 160, 60


@pytest.fixture(scope="module")
def lap():
    """the first 160 scans of the lap mapped on an archive-enabled handle, which stays open (tests only read it)"""
    hm = binding.Handle(_params())
    hm.map_enable(256, 1 << 20)
    track = np.zeros((N_MAP, 7))
    for k in range(N_MAP):
        flags, odom, mp = hm.scan_process(_scan(k), stages=7)
        track[k] = np.r_[mp["t"], mp["q"]]
    nf, dropped = hm.map_status()[:2]
    assert nf >= 8 and dropped == 0, (nf, dropped)
    out = dict(hm=hm, frames=_pull(hm), track=track)
    yield out
    hm.close()


def _loc_pair(lap, capacity=0):
    """(device route, host route) on the lap's archive, both placed at the mapping run's pose of scan N_MAP - 1"""
    a, b = binding.Handle(_params(K)), binding.Handle(_params(K))
    a.loc_enable_from_map(lap["hm"], 0, RADIUS, capacity)
    b.loc_enable(_tuples(lap["frames"]), RADIUS)
    for h in (a, b):
        _place(h, lap["track"][N_MAP - 1])
    return a, b


def _cmp_reloc(x, y, tag):
    assert len(x) == len(y)
    for rx, ry in zip(x, y):
        assert rx.keys() == ry.keys()
        for k in rx:
            assert_bit_equal(np.asarray(rx[k]), np.asarray(ry[k]), f"{tag} {k}")


@pytest.mark.gpu
def test_lap_localises_alike_after_either_route(lap):
    a, b = _loc_pair(lap)
    _assert_store_equal(a, b, len(lap["frames"]), "lap")
    ran = 0
    for k in range(N_MAP - 1, N_MAP - 1 + N_LOC):
        for h in (a, b):
            h.scan_process(_scan(k), stages=7)
        ran += int(a.debug_get("lm_info")[LI_RUN])
        _assert_state_equal(a, b, f"scan {k}")
    assert ran >= N_LOC // 2 - 1 and a.loc_status()["window"] > 0 and a.loc_status()["rebuilds"] >= 2, a.loc_status()
    for h in (a, b):
        h.reloc_enable()
    for name in ("rl_map_desc", "rl_map_key"):
        assert_bit_equal(a.debug_get(name), b.debug_get(name), name)
    _cmp_reloc(a.loc_relocalize([0]), b.loc_relocalize([0]), "relocalize")
    for h in (a, b):
        h.close()
    _guards_clean()


# ---- 3. the source is only read ----------------------------------------------------------------------------------------------
def _archive_snapshot(h):
    n = h.map_status()[0]
    return dict(status=h.map_status(), poses=np.array([h.map_get_keyframe(i)["pose"] for i in range(n)], F32), stamps=h.map_get_stamps(),
                cloud=h.map_assemble(binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER))


@pytest.mark.gpu
def test_the_source_is_only_read_and_keeps_mapping():
    n0, more = 60, 20
    hm, twin = binding.Handle(_params()), binding.Handle(_params())
    for h in (hm, twin):
        h.map_enable(64, 1 << 20)
        for k in range(n0):
            h.scan_process(_scan(k), stages=7)
    before = _archive_snapshot(hm)
    assert before["status"][0] >= 3
    a = binding.Handle(_params(K))
    a.loc_enable_from_map(hm, 0, RADIUS)
    after = _archive_snapshot(hm)
    assert before["status"] == after["status"]
    for name in ("poses", "stamps", "cloud"):
        assert_bit_equal(after[name], before[name], f"archive {name} after the hand-over")
    a.loc_update_from_map(hm)
    again = _archive_snapshot(hm)
    for name in ("poses", "stamps", "cloud"):
        assert_bit_equal(again[name], before[name], f"archive {name} after the update")
    for k in range(n0, n0 + more):
        for h in (hm, twin):
            h.scan_process(_scan(k), stages=7)
        assert_bit_equal(hm.debug_get("lm_state"), twin.debug_get("lm_state"), f"scan {k} lm_state")
        assert hm.lm_keyframe_count() == twin.lm_keyframe_count()
    assert hm.map_status() == twin.map_status()
    for h in (a, hm, twin):
        h.close()
    _guards_clean()


@pytest.mark.gpu
def test_a_keyframe_still_queued_is_handed_over():
    """alego_batch_run(.., sync = 0) returns with LaserMapping of the last scan in flight; the hand-over waits for it"""
    hq, hs = binding.Handle(_params()), binding.Handle(_params())
    for h in (hq, hs):
        h.map_enable(16, 1 << 18)
    for k in range(2):   # the second scan is the first mapping frame: it saves key frame 0
        hs.batch_load(0, 0, _scan(k))
        hs.batch_run(0, 1, stages=7, sync=True)
        hs.synchronize()
        hq.batch_load(0, 0, _scan(k))
        hq.batch_run(0, 1, stages=7, sync=False)
    a, b = binding.Handle(_params(K)), binding.Handle(_params(K))
    a.loc_enable_from_map(hq, 0, RADIUS)   # (no alego_synchronize in between)
    b.loc_enable_from_map(hs, 0, RADIUS)
    assert hs.map_status()[0] == 1 and a.loc_status()["frames"] == 1
    _assert_store_equal(a, b, 1, "queued key frame")
    for h in (a, b, hq, hs):
        h.close()
    _guards_clean()


# ---- 4. update ----------------------------------------------------------------------------------------------------------------
def _shifted(frames, d):
    out = []
    for f in frames:
        g = dict(f)
        g["pose"] = (f["pose"] + np.r_[d, 0, 0, 0].astype(F32)).astype(F32)
        out.append(g)
    return out


def _run(hs, lap, first, n, each=None):
    for k in range(first, first + n):
        for h in hs:
            h.scan_process(_scan(k), stages=7)
        if each:
            each(k)


@pytest.mark.gpu
def test_update_before_the_first_scan_equals_enabling_from_the_newer_archive(lap):
    frames = lap["frames"]
    n1 = len(frames) - 3
    m = _mapping_handle(frames[:n1])
    a = binding.Handle(_params(K))
    a.set_option("ALEGO_LOC_CHUNK", 5)
    a.loc_enable_from_map(m, 0, RADIUS, capacity=len(frames) + 2)
    for f in frames[n1:]:   # S2: more frames, some poses changed
        m.lm_add_keyframe(f["pose"], f["corner"], f["surf"], f["outlier"])
    m.map_set_keyposes(1, np.array([frames[1]["pose"], frames[2]["pose"]], F32) + F32(0.05))
    a.loc_update_from_map(m)
    b = binding.Handle(_params(K))
    b.loc_enable_from_map(m, 0, RADIUS)
    _assert_store_equal(a, b, len(frames), "updated before the first scan")
    for h in (a, b):
        _place(h, lap["track"][N_MAP - 1])
    _run((a, b), lap, N_MAP - 1, 40, lambda k: _assert_state_equal(a, b, f"scan {k}"))
    assert a.loc_status()["window"] > 0
    for h in (a, b, m):
        h.close()
    _guards_clean()


@pytest.mark.gpu
def test_update_mid_run_with_the_same_archive_changes_nothing_but_a_rebuild(lap):
    a, b = _loc_pair(lap)
    _run((a, b), lap, N_MAP - 1, 20)
    _assert_state_equal(a, b, "before the update")
    nonempty = a.loc_status()["window"] > 0
    assert nonempty
    m2o, params = a.debug_get("lm_state")[LD_M2O:LD_M2O + 7].copy(), a.debug_get("lm_state")[0:6].copy()
    lo = a.debug_get("lo_state").copy()
    a.loc_update_from_map(lap["hm"])
    s = a.loc_status()
    assert (s["frames"], s["window"]) == (len(lap["frames"]), 0), s
    st = a.debug_get("lm_state")
    assert_bit_equal(st[LD_M2O:LD_M2O + 7], m2o, "map -> odom across the update")
    assert_bit_equal(st[0:6], params, "params_ across the update")
    assert_bit_equal(a.debug_get("lo_state"), lo, "LaserOdometry state across the update")
    _assert_store_equal_frames(a, b, len(lap["frames"]), "same archive")

    mapped = []

    def each(k):
        mapped.append(bool(a.debug_get("lm_info")[LI_RUN]))
        if any(mapped):   # from the slot's next mapping frame on
            _assert_state_equal(a, b, f"scan {k}", rebuilds_ahead=1)
        else:             # until then the window is empty and the pose is the twin's
            assert a.loc_status()["window"] == 0
            assert_bit_equal(a.debug_get("lm_state"), b.debug_get("lm_state"), f"scan {k} lm_state")
    _run((a, b), lap, N_MAP + 19, 20, each)
    assert sum(mapped) >= 9
    _assert_state_equal(a, b, "end", rebuilds_ahead=1)
    for h in (a, b):
        h.close()
    _guards_clean()


def _assert_store_equal_frames(a, b, n, tag):
    for f in range(n):
        x, y = a.loc_store_frame(f), b.loc_store_frame(f)
        for name in x:
            assert_bit_equal(x[name], y[name], f"{tag} frame {f} {name}")
    assert_bit_equal(a.debug_get("lm_keyposes"), b.debug_get("lm_keyposes"), f"{tag} lm_keyposes")


@pytest.mark.gpu
def test_update_mid_run_to_an_archive_that_differs_out_of_reach(lap):
    frames = lap["frames"]
    far = dict(frames[0])
    far["pose"] = (frames[0]["pose"] + np.r_[1000, 1000, 0, 0, 0, 0].astype(F32)).astype(F32)
    m = _mapping_handle(frames)
    a, b = binding.Handle(_params(K)), binding.Handle(_params(K))
    a.loc_enable_from_map(m, 0, RADIUS, capacity=len(frames) + 1)
    b.loc_enable_from_map(m, 0, RADIUS)
    for h in (a, b):
        _place(h, lap["track"][N_MAP - 1])
    _run((a, b), lap, N_MAP - 1, 20)
    m.lm_add_keyframe(far["pose"], far["corner"], far["surf"], far["outlier"])
    a.loc_update_from_map(m)
    assert a.loc_status()["frames"] == len(frames) + 1
    kp1 = np.array([f["pose"] for f in frames], F32)
    kp2 = np.r_[kp1, far["pose"][None]]
    seen = []

    def each(k):
        if not a.debug_get("lm_info")[LI_RUN]:
            return
        p = a.debug_get("lm_state")[LD_LOC_P:LD_LOC_P + 3].astype(F32)
        w1, w2 = binding.loc_select(kp1, p, RADIUS, K), binding.loc_select(kp2, p, RADIUS, K)
        assert np.array_equal(w1, w2), "the premise: the new frame is out of reach of every position"
        assert np.array_equal(a.debug_get("lm_window"), w2) and np.array_equal(w2, select_np(kp2, p, RADIUS, K)), (k, w2)
        seen.append(len(w2))
        for name in STATE:
            assert_bit_equal(a.debug_get(name), b.debug_get(name), f"scan {k} {name}")
        assert a.loc_status()["rebuilds"] == b.loc_status()["rebuilds"] + 1
    _run((a, b), lap, N_MAP + 19, 20, each)
    assert len(seen) >= 8 and min(seen) > 0
    for h in (a, b, m):
        h.close()
    _guards_clean()


@pytest.mark.gpu
def test_update_mid_run_to_a_moved_archive(lap):
    from test_gpu_parity import POSE_TOL, _lm_compare
    frames = lap["frames"]
    moved = _shifted(frames, [0.3, 0.0, 0.0])
    m = _mapping_handle(frames)
    pl = _params(K)
    a = binding.Handle(pl)
    a.loc_enable_from_map(m, 0, RADIUS)
    a.reloc_enable()
    _place(a, lap["track"][N_MAP - 1])
    _run((a,), lap, N_MAP - 1, 20)
    assert a.loc_status()["window"] > 0
    m.map_set_keyposes(0, np.array([f["pose"] for f in moved], F32))
    a.loc_update_from_map(m)
    fresh = binding.Handle(pl)
    fresh.loc_enable_from_map(m, 0, RADIUS)
    fresh.reloc_enable()
    _assert_store_equal_frames(a, fresh, len(frames), "moved archive")
    for name in ("rl_map_desc", "rl_map_key"):
        assert_bit_equal(a.debug_get(name), fresh.debug_get(name), name)
    assert a.loc_status()["window"] == 0 and a.loc_status()["frames"] == len(frames)
    kp2 = np.array([f["pose"] for f in moved], F32)
    k, checked = N_MAP + 19, 0
    while not checked:
        st0 = a.debug_get("lm_state")
        flags, odom, mp, seg, feat = a.scan_process(_scan(k), stages=7, want_outputs=True)
        gi = a.debug_get("lm_info")
        if gi[LI_RUN]:
            st1 = a.debug_get("lm_state")
            win = a.debug_get("lm_window")
            assert len(win) > 0
            assert np.array_equal(win, binding.loc_select(kp2, st1[LD_LOC_P:LD_LOC_P + 3].astype(F32), RADIUS, K)), win
            e = emulate(pl, moved, win, st0[LD_M2O:LD_M2O + 7], st0[0:6], feat["less_sharp"], feat["less_flat"], seg["outlier"], np.r_[odom["t"], odom["q"]])
            _lm_compare(_WindowAsKeyFrames(a, len(win)), e, k, f"moved archive scan {k}")
            want = e.get("map_pose")
            assert np.abs(mp["t"] - want[:3]).max() < POSE_TOL and quat_angle(mp["q"], want[3:]) < POSE_TOL, (mp["t"], want)
            e.close()
            checked += 1
        k += 1
        assert k < N_MAP + 24
    for h in (a, fresh, m):
        h.close()
    _guards_clean()


@pytest.mark.gpu
def test_a_shrinking_update_leaves_no_window_beyond_the_new_frames(lap):
    frames = lap["frames"]
    n2, radius = len(frames) - 2, 2 * RADIUS   # (the newest two frames go; the wider radius keeps older ones in reach)
    m1, m2 = _mapping_handle(frames), _mapping_handle(frames[:n2])
    a, b = binding.Handle(_params(K)), binding.Handle(_params(K))
    a.loc_enable_from_map(m1, 0, radius)
    b.loc_enable_from_map(m2, 0, radius)
    _place(a, lap["track"][N_MAP - 1])
    _run((a,), lap, N_MAP - 1, 20)
    assert a.debug_get("lm_window").max() >= n2, "the premise: the window named a frame the update drops"
    a.loc_update_from_map(m2)
    _assert_store_equal_frames(a, b, n2, "shrunk")
    assert a.loc_status()["frames"] == n2

    def each(k):
        w = a.debug_get("lm_window")
        assert len(w) == 0 or w.max() < n2, (k, w)
    _run((a,), lap, N_MAP + 19, 20, each)
    assert a.loc_status()["window"] > 0
    for h in (a, b, m1, m2):
        h.close()
    _guards_clean()


@pytest.mark.gpu
def test_update_between_two_batch_runs_of_128_slots(lap):
    """128 slots in two stream groups replay from the bag store and are updated between two alego_batch_run calls (the first without a
    synchronisation); slots 0, 63, 64 and 127 equal one-slot replicas updated at the same scan."""
    frames, track = lap["frames"], lap["track"]
    m1, m2 = _mapping_handle(frames), _mapping_handle(_shifted(frames, [0.0, 0.1, 0.0]))
    pl = _params(K)
    n_slots, half, nbag = 128, 20, N_MAP
    start = lambda s: 60 + (s * 7) % 60

    def replay(starts, sync):
        h = binding.Handle(pl, n_slots=len(starts))
        h.replay_create(1, nbag)
        for k in range(nbag):
            h.replay_load(0, k, _scan(k))
        h.trajectory_enable(2 * half)
        h.loc_enable_from_map(m1, 0, RADIUS)
        for s, st in enumerate(starts):
            h.replay_assign(s, 0, st)
            _place(h, track[st], slot=s)
        h.batch_run(0, half, stages=7 | binding.REPLAY_BAG, sync=sync)
        h.loc_update_from_map(m2)
        h.batch_run(half, half, stages=7 | binding.REPLAY_BAG, sync=sync)
        h.synchronize()
        return h

    h = replay([start(s) for s in range(n_slots)], False)
    groups, per = h.stream_groups()
    assert groups >= 2
    for s in (0, 63, 64, 127):
        r = replay([start(s)], True)
        assert_bit_equal(h.trajectory(s), r.trajectory(0), f"slot {s} trajectory log")
        for name in STATE + ("lm_info",):
            assert_bit_equal(h.debug_get(name, slot=s), r.debug_get(name), f"slot {s} {name}")
        assert h.loc_status(s) == r.loc_status(0) and h.loc_status(s)["window"] > 0, (s, h.loc_status(s))
        r.close()
    for x in (h, m1, m2):
        x.close()
    _guards_clean()


# ---- 5. misuse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misuse_is_refused_and_leaves_the_handles_as_they_were(lap):
    frames = lap["frames"]
    n = len(frames)
    m = _mapping_handle(frames, n_slots=2)
    plain = binding.Handle(_params())   # no archive
    ARG, CAPACITY = binding.ERR_ARG, binding.ERR_CAPACITY
    a = binding.Handle(_params(K))
    for map_, slot in ((None, 0), (a, 0), (plain, 0), (m, 2), (m, -1)):
        _refused(lambda: a.loc_enable_from_map(map_, slot, RADIUS), ARG)
    _refused(lambda: a.loc_update_from_map(m, 0), ARG, "does not localise")
    _refused(lambda: a.loc_enable_from_map(m, 0, RADIUS, capacity=n - 1), CAPACITY)
    _refused(lambda: a.loc_enable_from_map(m, 0, RADIUS, capacity=8193), CAPACITY)
    # a frame beyond the handle's key-frame capacities, named with its counts
    small = _params(K, kf_cap_surf=500, kf_cap_outlier=7200)
    big_i = next(i for i, f in enumerate(frames) if len(f["surf"]) > 500)
    c = binding.Handle(small)
    _refused(lambda: c.loc_enable_from_map(m, 0, RADIUS), CAPACITY, f"frame {big_i} ({len(frames[big_i]['corner'])} corner, {len(frames[big_i]['surf'])} surf")
    c.close()
    # the preconditions of alego_loc_enable
    used = binding.Handle(_params(K))
    used.scan_process(_scan(0), stages=7)
    _refused(lambda: used.loc_enable_from_map(m, 0, RADIUS), ARG, "before the first scan")
    used.close()
    other = _mapping_handle(frames[:1])
    _refused(lambda: m.loc_enable_from_map(other, 0, RADIUS), ARG, "belong to a mapping handle")
    other.close()
    # after every refusal the handle is the SLAM handle it was: it can still be enabled, and then localises like a twin
    a.loc_enable_from_map(m, 0, RADIUS)
    _refused(lambda: a.loc_enable_from_map(m, 0, RADIUS), ARG, "already enabled")
    twin = binding.Handle(_params(K))
    twin.loc_enable_from_map(m, 0, RADIUS)
    for h in (a, twin):
        _place(h, lap["track"][N_MAP - 1])
    _run((a, twin), lap, N_MAP - 1, 10)
    # updates that are refused before anything is written
    m.lm_add_keyframe(frames[0]["pose"], frames[0]["corner"], frames[0]["surf"], frames[0]["outlier"])
    _refused(lambda: a.loc_update_from_map(m, 0), CAPACITY, "capacity")   # n + 1 frames, capacity n
    over = _mapping_handle([(frames[0]["pose"], np.zeros((CAP_C, 4), F32), np.zeros((CAP_S, 4), F32), EMPTY)])
    s, tiny = binding.Handle(small), _mapping_handle([(frames[0]["pose"], EMPTY, EMPTY, EMPTY)])
    s.loc_enable_from_map(tiny, 0, RADIUS)
    _refused(lambda: s.loc_update_from_map(over, 0), CAPACITY, "frame 0")
    assert s.loc_status()["frames"] == 1
    s.close()
    tiny.close()
    for map_, slot in ((None, 0), (a, 0), (plain, 0), (m, 2), (m, -1)):
        _refused(lambda: a.loc_update_from_map(map_, slot), ARG)
    _run((a, twin), lap, N_MAP + 9, 10, lambda k: _assert_state_equal(a, twin, f"scan {k} after the refused calls"))
    assert a.loc_status()["window"] > 0
    # a store built by alego_loc_enable has the capacity of its frames: an update to fewer frames works, to more is refused
    old = binding.Handle(_params(K))
    old.loc_enable(_tuples(frames), RADIUS)
    _refused(lambda: old.loc_update_from_map(m, 0), CAPACITY)
    fewer = _mapping_handle(frames[:n - 2])
    old.loc_update_from_map(fewer, 0)
    assert old.loc_status()["frames"] == n - 2
    for h in (a, twin, old, fewer, over, m, plain):
        h.close()
    _guards_clean()


# ---- 6. examples/replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cpp_example_hands_its_archive_over_on_the_device():
    exe = os.path.join(ROOT, "examples", "replay")
    host = subprocess.run([exe, "200", "--localize"], capture_output=True, text=True, timeout=600)
    dev = subprocess.run([exe, "200", "--localize", "--on-device"], capture_output=True, text=True, timeout=600)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    jh, jd = json.loads(host.stdout.strip().splitlines()[-1]), json.loads(dev.stdout.strip().splitlines()[-1])
    assert jd["loc_on_device"] == 1 and jh.get("loc_on_device", 0) == 0
    for key in ("loc_frames", "loc_map_t", "loc_max_dev"):
        assert jd[key] == jh[key], (key, jd[key], jh[key])   # the printed digits
    # the same hand-over through the binding
    p = _params()
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    track = []
    for k in range(200):
        flags, odom, mp = h.scan_process(_scan(k), stages=7, stamp=0.1 * k)
        track.append(mp["t"].copy())
    assert jd["loc_frames"] == h.map_status()[0]
    hl = binding.Handle(p)
    hl.loc_enable_from_map(h, 0, 0.0)
    dev_max = 0.0
    for k in range(200):
        flags, odom, mp = hl.scan_process(_scan(k), stages=7, stamp=0.1 * k)
        dev_max = max(dev_max, np.abs(mp["t"] - track[k]).max())
    assert [float(v) for v in mp["t"]] == jd["loc_map_t"], (mp["t"], jd["loc_map_t"])
    assert float(f"{dev_max:.9g}") == jd["loc_max_dev"], (dev_max, jd["loc_max_dev"])
    for x in (h, hl):
        x.close()
    _guards_clean()
