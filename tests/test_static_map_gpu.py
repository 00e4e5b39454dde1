"""The static map (alego_occ_mark, alego_map_assemble_static) on the device.

Archives are built with alego_lm_add_keyframe from hand-made clouds.  In every case the verdicts and stats of alego_occ_mark are compared for EXACT
equality with the host twin alego_occ_mark_host on the points of alego_map_assemble(kinds | ALEGO_MAP_FRAME_ID, leaf 0), the sensor-frame z of
alego_map_get_keyframe and the counts of alego_occ_get (the twin itself stands against tests/static_ref.py in tests/test_static_math.py), and
alego_map_assemble_static(leaf 0) with raw[verdict != REMOVED] bit for bit, with and without ALEGO_MAP_FRAME_ID."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from static_ref import SCENE_GRID, scene
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
FID = binding.MAP_FRAME_ID
REMOVED = binding.STATIC_REMOVED
G0 = dict(origin=(-8.0, -8.0, -2.0), cell=(0.4, 0.4, 0.5), n=(40, 40, 8))   # 16 m x 16 m x 4 m around the sensors
NONE = np.zeros((0, 4), np.float32)
SR = binding.static_rule
RULES = (None, SR(protect_radius=1), SR(occ=(1, 1, 2), protect_radius=2, keep_below=-0.5))


def _err(h):
    return binding.lib().alego_last_error(h._h).decode()


def _cloud(rng, n, spread=(9.0, 9.0, 1.5)):
    """n points of the sensor frame, uniform in +/- spread: a part of them leaves G0"""
    return np.concatenate([rng.uniform(-1, 1, (n, 3)) * np.array(spread), rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)


def _frame(rng, pose, nc, ns, no, **kw):
    return dict(pose=np.asarray(pose, np.float32), corner=_cloud(rng, nc, **kw), surf=_cloud(rng, ns, **kw), outlier=_cloud(rng, no, **kw))


def _handle(p, opts, frames, n_slots=1, map_frames=16, map_points=1 << 14):
    """frames: {slot: [frame, ...]}"""
    h = binding.Handle(p, n_slots=n_slots)
    h.map_enable(map_frames, map_points)
    for s, fl in frames.items():
        for fr in fl:
            h.lm_add_keyframe(fr["pose"], fr["corner"], fr["surf"], fr["outlier"], slot=s)
    if opts is not None:
        h.occ_enable(opts)
    return h


def _sensor_z(h, kinds, slot=0):
    """the archived z of every selected point in assembly order: frames ascending, within a frame surf, corner, outlier"""
    z = [np.zeros(0, np.float32)]
    for f in range(h.map_status(slot)[0]):
        kf = h.map_get_keyframe(f, slot)
        z += [kf[name][:, 2] for bit, name in ((binding.MAP_SURF, "surf"), (binding.MAP_CORNER, "corner"), (binding.MAP_OUTLIER, "outlier")) if kinds & bit]
    return np.concatenate(z)


def _check(h, opts, tag, kinds=ALL, rule=None, slot=0, sensor_z=None):
    """mark and both static assemblies against the twin and the raw assembly; returns (raw with frame ids, verdicts, stats)"""
    raw = h.map_assemble(kinds | FID, 0.0, slot=slot)
    sz = _sensor_z(h, kinds, slot) if sensor_z is None else sensor_z
    assert sz.shape[0] == raw.shape[0]
    hits, passes = h.occ_get()
    want_v, want_s = binding.occ_mark_host(opts, hits, passes, raw, rule, sz)
    v, s = h.occ_mark(kinds, rule, slot)
    bad = np.nonzero(v != want_v)[0] if v.shape == want_v.shape else None
    assert bad is not None and bad.size == 0, f"{tag}: verdicts differ at {None if bad is None else bad[:5].tolist()} of {want_v.shape[0]} (got {v.shape[0]})"
    assert np.array_equal(s, want_s), f"{tag}: stats {s.tolist()} want {want_s.tolist()}"
    v2, _ = h.occ_mark(kinds | FID, rule, slot)
    assert np.array_equal(v2, v), f"{tag}: ALEGO_MAP_FRAME_ID changes no verdict"
    plain = h.map_assemble(kinds, 0.0, slot=slot)
    for k, src in ((kinds | FID, raw), (kinds, plain)):
        out, s2 = h.map_assemble_static(k, 0.0, rule, slot)
        assert_bit_equal(out, src[v != REMOVED], f"{tag}: static assembly, kinds {k}")
        assert np.array_equal(s2, want_s), f"{tag}: static assembly's stats"
    return raw, v, s


def _integrate(h, kinds=ALL, slot=0):
    h.occ_clear()
    h.occ_integrate(kinds, slot=slot)


@pytest.mark.gpu
@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 255, 256, 257, 513])
def test_one_frame(params_a, n_points):
    rng = np.random.default_rng(100 + n_points)
    opts = binding.occ_opts(**G0)
    h = _handle(params_a, opts, {0: [_frame(rng, (0.3, -0.2, 0.1, 0.02, -0.03, 0.4), 0, n_points, 0)]})
    _integrate(h)
    for i, rule in enumerate(RULES):
        _, v, s = _check(h, opts, f"{n_points} points, rule {i}", rule=rule)
        assert v.shape[0] == n_points == s.sum()
        print(f"{n_points} points, rule {i}: stats {s.tolist()}")
    h.close()


@pytest.fixture(scope="module")
def three_frames(params_a):
    """3 frames with rotated poses; each has one empty cloud, frame 1 straddles a chunk (300 selected points); integrated once, all kinds"""
    rng = np.random.default_rng(7)
    frames = [_frame(rng, (0.5, 0.25, 0.0, 0.05, -0.1, 0.7), 0, 90, 40), _frame(rng, (-2.0, 1.5, 0.3, -0.2, 0.1, -2.5), 130, 0, 170),
              _frame(rng, (3.0, -3.5, -0.4, 0.3, 0.25, 3.0), 60, 45, 0)]
    opts = binding.occ_opts(**G0)
    h = _handle(params_a, opts, {0: frames})
    _integrate(h)
    yield h, opts
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", range(1, 8))
def test_each_kinds_mask(three_frames, kinds):
    h, opts = three_frames
    want = sum(n for bit, n in ((binding.MAP_CORNER, 0 + 130 + 60), (binding.MAP_SURF, 90 + 0 + 45), (binding.MAP_OUTLIER, 40 + 170 + 0)) if kinds & bit)
    seen = np.zeros(binding.STATIC_VERDICTS, np.int64)
    for i, rule in enumerate(RULES):
        _, v, s = _check(h, opts, f"kinds {kinds}, rule {i}", kinds=kinds, rule=rule)
        assert v.shape[0] == want
        seen += s
    if kinds == ALL:
        print(f"three frames: verdicts over the rules {seen.tolist()}")
        assert (seen[[binding.STATIC_OCCUPIED, binding.STATIC_OUTSIDE, binding.STATIC_BELOW, binding.STATIC_NEIGHBOUR, REMOVED]] > 0).all()


# ---- removal patterns: the verdict of every point is set by its sensor-frame z
# The frame's surf points all lie in the cell of the key pose itself, one outlier point far away: the cell takes N hits and 1 pass, which the rule
# (1, 1, 1000) calls free.  keep_below 0 then keeps exactly the points with z < 0 (BELOW) and removes the others; kinds = SURF leaves the outlier out.
PATTERNS = {
    "everything_removed": (300, lambda i: np.zeros_like(i, bool)),
    "nothing_removed": (300, lambda i: np.ones_like(i, bool)),
    "last_lane_of_each_chunk": (512, lambda i: i % 256 == 255),
    "lane_0_of_each_wavefront": (600, lambda i: i % 64 == 0),
    "an_empty_item_between_two": (700, lambda i: (i < 256) | (i >= 512)),
    "all_but_lane_0": (257, lambda i: i % 256 != 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_removal_patterns(params_a, name):
    n, keep_of = PATTERNS[name]
    keep = keep_of(np.arange(n))
    rng = np.random.default_rng(len(name))
    surf = np.concatenate([rng.uniform(-0.1, 0.1, (n, 2)), np.where(keep, -1.0, 1.0)[:, None] * rng.uniform(0.01, 0.1, (n, 1)), np.zeros((n, 1))], axis=1).astype(np.float32)
    far = np.array([[5.0, 3.0, 0.5, 0]], np.float32)
    # two such frames: the patterns repeat, and the second frame's items follow items that kept other numbers of points
    frames = [dict(pose=np.array([0.2, 0.2, 0.25, 0, 0, 0], np.float32), corner=NONE, surf=surf, outlier=far),
              dict(pose=np.array([-3.8, 2.2, -0.25, 0, 0, 0], np.float32), corner=NONE, surf=surf[::-1].copy(), outlier=far)]
    opts = binding.occ_opts(**G0)
    h = _handle(params_a, opts, {0: frames})
    _integrate(h)
    rule = SR(occ=(1, 1, 1000), keep_below=0.0)
    raw, v, s = _check(h, opts, name, kinds=binding.MAP_SURF, rule=rule)
    both = np.concatenate([keep, keep[::-1]])
    assert np.array_equal(v != REMOVED, both) and s[binding.STATIC_BELOW] == both.sum() and s[REMOVED] == (~both).sum() and s.sum() == 2 * n
    L = binding.lib()
    out = np.full((2 * n + 8, 4), -7.0, np.float32)
    got = L.alego_map_assemble_static(h._h, 0, binding.MAP_SURF, 0.0, C.byref(rule), out.ctypes.data, out.shape[0], None)
    assert got == both.sum() and (out[got:] == -7.0).all(), "nothing is written behind the kept points"
    if name == "everything_removed":
        assert got == 0
    if name == "nothing_removed":
        assert_bit_equal(out[:got], h.map_assemble(binding.MAP_SURF), "nothing removed: alego_map_assemble's cloud")
    h.close()


@pytest.mark.gpu
def test_item_counts_across_the_scan_rounds(params_a):
    """occ_offsets scans 1 024 items per round with a carry: 1 025 and 2 049 frames of one surf point each, every third removed.  Frame f sits in row
    f of the grid and looks along x; every third frame also holds three outlier points further along the same ray, whose passes free the surf point's cell."""
    opts = binding.occ_opts(origin=(0.0, 0.0, 0.0), cell=(1.0, 1.0, 1.0), n=(8, 2049, 1))
    h = binding.Handle(params_a)
    h.map_enable(2049, 8192)
    h.occ_enable(opts)
    surf = np.array([[3.0, 0.0, 0.0, 0.0]], np.float32)
    beyond = np.array([[6.0, 0.0, 0.0, 0.0]] * 3, np.float32)
    done = 0
    for n_frames in (1025, 2049):
        for f in range(done, n_frames):
            h.lm_add_keyframe(np.array([0.5, f + 0.5, 0.5, 0, 0, 0], np.float32), NONE, surf, beyond if f % 3 == 0 else NONE)
        done = n_frames
        _integrate(h)
        raw, v, s = _check(h, opts, f"{n_frames} frames", kinds=binding.MAP_SURF, sensor_z=np.zeros(n_frames, np.float32))
        assert v.shape[0] == n_frames and np.array_equal(v == REMOVED, np.arange(n_frames) % 3 == 0) and s[binding.STATIC_OCCUPIED] == n_frames - s[REMOVED]
        out, _ = h.map_assemble_static(binding.MAP_SURF | FID)
        assert np.array_equal(out[:, 3], np.arange(n_frames, dtype=np.float32)[np.arange(n_frames) % 3 != 0])
    _check(h, opts, "2 049 frames, all kinds", sensor_z=np.zeros(2049 + 3 * 683, np.float32))
    h.close()


GRIDS = {
    "small_grid_faces_edges_corners": dict(origin=(-1.5, -1.25, -1.0), cell=(0.5, 0.5, 0.5), n=(6, 5, 4)),
    "one_cell": dict(origin=(-0.5, -0.5, -0.5), cell=(1.5, 1.5, 1.0), n=(1, 1, 1)),
    "holds_no_point": dict(origin=(40.0, 40.0, 5.0), cell=(0.4, 0.4, 0.4), n=(10, 10, 10)),
    "with_ranges": dict(origin=(-8.0, -8.0, -2.0), cell=(0.4, 0.4, 0.5), n=(40, 40, 8), min_range=3.0, max_range=7.0),
    "odd_cells": dict(origin=(-7.7, -8.3, -1.9), cell=(0.37, 0.53, 0.71), n=(43, 31, 5)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grids_and_rules(params_a, name):
    rng = np.random.default_rng(11)
    opts = binding.occ_opts(**GRIDS[name])
    spread = dict(spread=(1.6, 1.4, 1.1)) if name == "small_grid_faces_edges_corners" else {}
    frames = [_frame(rng, (0.2, 0.1, 0.0, 0.0, 0.0, 0.3), 50, 200, 50, **spread), _frame(rng, (0.6, -0.3, 0.1, 0.1, -0.05, -1.0), 40, 120, 30, **spread)]
    h = _handle(params_a, opts, {0: frames})
    _integrate(h)
    seen, at_faces = np.zeros(binding.STATIC_VERDICTS, np.int64), set()
    for i, rule in enumerate(RULES + (SR(occ=(1, 1, 1), protect_radius=1), SR(occ=(2, 1, 1), protect_radius=2), SR(occ=(0, 0, 0)))):
        raw, v, s = _check(h, opts, f"{name}, rule {i}", rule=rule)
        seen += s
        if rule is not None and rule.protect_radius > 0:
            n = np.array(opts.n[:])
            c = np.floor((raw[:, :3].astype(np.float64) - np.array(opts.origin[:])) / np.array(opts.cell[:]))
            judged = (v == binding.STATIC_NEIGHBOUR) | (v == REMOVED)       # the points whose neighbourhood was read
            at_faces |= set(((c == 0) | (c == n - 1)).sum(axis=1)[judged].tolist())
    print(f"{name}: verdicts over the rules {seen.tolist()}")
    if name == "small_grid_faces_edges_corners":
        assert {1, 2, 3} <= at_faces, "neighbourhoods were read from face, edge and corner cells"
    if name == "holds_no_point":
        assert seen[binding.STATIC_OUTSIDE] == seen.sum()
    if name == "with_ranges":
        assert seen[binding.STATIC_UNKNOWN] > 0   # truncated rays: end cells nobody visited
    h.close()


@pytest.mark.gpu
def test_non_finite_points(params_a):
    opts = binding.occ_opts(**G0)
    rng = np.random.default_rng(5)
    fr = _frame(rng, (0, 0, 0, 0, 0, 0), 0, 70, 0)
    fr["surf"][3, 0] = np.nan; fr["surf"][17, 2] = np.inf; fr["surf"][40, 1] = 3.0e9; fr["surf"][41, 1] = -np.inf
    h = _handle(params_a, opts, {0: [fr]})
    _integrate(h)
    for rule in RULES:
        _, v, _ = _check(h, opts, "non-finite and far points", rule=rule)
        assert (v[[3, 17, 40, 41]] == binding.STATIC_OUTSIDE).all()
    h.close()


@pytest.mark.gpu
def test_moved_key_pose_is_judged_where_the_points_are_now(three_frames):
    h, opts = three_frames
    rule = SR(protect_radius=1)
    _, before, _ = _check(h, opts, "before the move", rule=rule)
    old = np.concatenate([h.map_get_keyframe(1)["pose"]])
    h.map_set_keyposes(1, np.array([[1.5, 2.5, -0.2, 0.1, 0.2, 1.0]], np.float32))
    _, after, _ = _check(h, opts, "after alego_map_set_keyposes, counts as they stood", rule=rule)
    assert not np.array_equal(before, after)
    h.map_set_keyposes(1, old[None, :])
    _, back, _ = _check(h, opts, "moved back", rule=rule)
    assert np.array_equal(back, before)


@pytest.mark.gpu
def test_slots(params_a, monkeypatch):
    """slot 1 of a 3-slot handle (two stream groups) gives what a one-slot replica gives"""
    rng = np.random.default_rng(21)
    fa = [_frame(rng, (0.5, 0.5, 0, 0, 0, 0.5), 30, 100, 20), _frame(rng, (-1, 1, 0.2, 0.1, 0, -0.5), 10, 80, 40)]
    fb = [_frame(rng, (2.0, -2.0, 0.1, 0, 0.1, 2.0), 64, 64, 64)]
    opts = binding.occ_opts(**G0)
    monkeypatch.setenv("ALEGO_STREAM_GROUPS", "2")
    h = _handle(params_a, opts, {1: fa, 2: fb}, n_slots=3)
    monkeypatch.delenv("ALEGO_STREAM_GROUPS")
    assert h.stream_groups()[0] == 2
    r = _handle(params_a, opts, {0: fa})
    _integrate(r)
    _integrate(h, slot=1)
    rule = SR(protect_radius=1)
    raw_r, v_r, s_r = _check(r, opts, "replica", rule=rule)
    raw_h, v_h, s_h = _check(h, opts, "slot 1 of 3", rule=rule, slot=1)
    assert_bit_equal(raw_h, raw_r, "slot 1 against the replica: raw")
    assert np.array_equal(v_h, v_r) and np.array_equal(s_h, s_r)
    _check(h, opts, "slot 2 against slot 1's counts", rule=rule, slot=2)
    _, v0, s0 = _check(h, opts, "the empty slot 0", rule=rule, slot=0)
    assert v0.shape[0] == 0 and s0.sum() == 0 and h.map_assemble_static(ALL, 0.4, rule, 0)[0].shape[0] == 0
    h.close(); r.close()


@pytest.mark.gpu
def test_leaf_count_only_and_capacity(three_frames):
    h, opts = three_frames
    L = binding.lib()
    rule = SR(protect_radius=1)
    raw, v, s = _check(h, opts, "leaf 0", rule=rule)
    kept = raw[v != REMOVED]
    assert 0 < kept.shape[0] < raw.shape[0]
    for kinds, src in ((ALL | FID, kept), (ALL, h.map_assemble(ALL)[v != REMOVED])):
        out, s2 = h.map_assemble_static(kinds, 0.4, rule)
        assert_bit_equal(out, h.voxel_grid_large(src, 0.4), f"leaf 0.4, kinds {kinds}: alego_voxel_grid of the static raw cloud")
        assert 0 < out.shape[0] < kept.shape[0] and np.array_equal(s2, s)
    # count only: the kernels run, stats are filled, nothing else is written
    stats = np.full(binding.STATIC_VERDICTS, -1, np.int64)
    assert L.alego_occ_mark(h._h, 0, ALL, C.byref(rule), None, 0, stats.ctypes.data) == raw.shape[0] and np.array_equal(stats, s)
    stats[:] = -1
    assert L.alego_map_assemble_static(h._h, 0, ALL, 0.0, C.byref(rule), None, 0, stats.ctypes.data) == kept.shape[0] and np.array_equal(stats, s)
    assert L.alego_map_assemble_static(h._h, 0, ALL, 0.4, C.byref(rule), None, 0, None) == h.voxel_grid_large(kept, 0.4).shape[0]
    assert L.alego_occ_mark(h._h, 0, ALL, None, None, 0, None) == raw.shape[0]                                   # rule and stats may be NULL
    # too small a cap: ALEGO_ERR_CAPACITY, the output untouched
    vb = np.full(raw.shape[0], 77, np.uint8)
    assert L.alego_occ_mark(h._h, 0, ALL, C.byref(rule), vb.ctypes.data, raw.shape[0] - 1, None) == binding.ERR_CAPACITY and (vb == 77).all() and "capacity" in _err(h)
    assert L.alego_occ_mark(h._h, 0, ALL, C.byref(rule), vb.ctypes.data, raw.shape[0], None) == raw.shape[0] and np.array_equal(vb, v)
    for leaf, n in ((0.0, kept.shape[0]), (0.4, h.voxel_grid_large(kept, 0.4).shape[0])):
        ob = np.full((raw.shape[0], 4), -7.0, np.float32)
        assert L.alego_map_assemble_static(h._h, 0, ALL, leaf, C.byref(rule), ob.ctypes.data, n - 1, None) == binding.ERR_CAPACITY and (ob == -7.0).all(), leaf
        assert L.alego_map_assemble_static(h._h, 0, ALL, leaf, C.byref(rule), ob.ctypes.data, n, None) == n and (ob[n:] == -7.0).all(), leaf
    # the archive and alego_map_assemble are what they were
    assert_bit_equal(h.map_assemble(ALL | FID), raw, "the raw assembly afterwards")


@pytest.mark.gpu
def test_every_refusal(params_a):
    L = binding.lib()
    rng = np.random.default_rng(2)
    opts = binding.occ_opts(**G0)
    stats, vb, ob = np.zeros(binding.STATIC_VERDICTS, np.int64), np.zeros(64, np.uint8), np.zeros((64, 4), np.float32)

    def calls(h, slot=0, kinds=ALL, rule=None):
        r = None if rule is None else C.byref(rule)
        return (L.alego_occ_mark(h._h, slot, kinds, r, vb.ctypes.data, 64, stats.ctypes.data),
                L.alego_map_assemble_static(h._h, slot, kinds, 0.0, r, ob.ctypes.data, 64, stats.ctypes.data))

    h = binding.Handle(params_a, n_slots=2)
    assert calls(h) == (binding.ERR_ARG,) * 2 and "archive is off" in _err(h)                                    # archive off
    h.map_enable(8, 4096)
    assert calls(h) == (binding.ERR_ARG,) * 2 and "alego_occ_enable" in _err(h)                                  # grid off
    for fr in (_frame(rng, (0, 0, 0, 0, 0, 0), 5, 5, 5), _frame(rng, (1, 0, 0, 0, 0, 0), 5, 5, 5)):
        h.lm_add_keyframe(fr["pose"], fr["corner"], fr["surf"], fr["outlier"])
    h.occ_enable(opts)
    h.occ_integrate()
    assert calls(h)[0] == 30 and calls(h, slot=1) == (0, 0) and calls(h, kinds=ALL | FID)[0] == 30
    for rule, word in ((SR(occ=(-1, 2, 1)), "negative"), (SR(occ=(1, -2, 1)), "negative"), (SR(occ=(1, 2, -1)), "negative"), (SR(protect_radius=-1), "protect_radius"),
                       (SR(protect_radius=3), "protect_radius"), (SR(keep_below=np.nan), "keep_below"), (SR(keep_below=-np.inf), "keep_below")):
        assert calls(h, rule=rule) == (binding.ERR_ARG,) * 2 and word in _err(h), word
    for kinds in (0, 8, 16, 16 | ALL, -1):
        assert calls(h, kinds=kinds) == (binding.ERR_ARG,) * 2 and "kinds" in _err(h), kinds
    for slot in (-1, 2):
        assert calls(h, slot=slot) == (binding.ERR_ARG,) * 2, slot
    assert L.alego_occ_mark(None, 0, ALL, None, None, 0, None) == binding.ERR_ARG and L.alego_map_assemble_static(None, 0, ALL, 0.0, None, None, 0, None) == binding.ERR_ARG
    assert L.alego_occ_mark(h._h, 0, ALL, None, None, 8, None) == binding.ERR_ARG and L.alego_occ_mark(h._h, 0, ALL, None, vb.ctypes.data, -1, None) == binding.ERR_ARG
    assert L.alego_map_assemble_static(h._h, 0, ALL, 0.0, None, ob.ctypes.data, -1, None) == binding.ERR_ARG
    h.close()
    # a localising handle is refused by the gate
    fr = _frame(rng, (0, 0, 0, 0, 0, 0), 20, 60, 20)
    h = binding.Handle(params_a)
    h.loc_enable([(fr["pose"], fr["corner"], fr["surf"], fr["outlier"])])
    assert calls(h) == (binding.ERR_ARG,) * 2 and "localising" in _err(h)
    h.close()


@pytest.mark.gpu
def test_scene_on_the_device(params_a):
    """the wall every key pose sees stays, the box each frame sees somewhere else goes (tests/test_static_math.py has the scene)"""
    kp, pts, is_box = scene()
    opts = binding.occ_opts(*SCENE_GRID)
    h = binding.Handle(params_a)
    h.map_enable(8, 1 << 14)
    for k in range(6):
        mine = pts[pts[:, 3] == k]
        local = np.concatenate([mine[:, :3] - kp[k, :3], np.zeros((mine.shape[0], 1), np.float32)], axis=1).astype(np.float32)
        h.lm_add_keyframe(np.array([*kp[k, :3], 0, 0, 0], np.float32), NONE, local, NONE)
    h.occ_enable(opts)
    stats = h.occ_integrate()
    assert stats[binding.OCC_RAYS] == 8766 and stats[1:5].sum() == 0
    for r in (0, 1):
        raw, v, s = _check(h, opts, f"scene, protect_radius {r}", kinds=binding.MAP_SURF, rule=SR(protect_radius=r))
        assert np.abs(raw[:, :3] - pts[:, :3]).max() < 1e-5 and np.array_equal(raw[:, 3], pts[:, 3])
        print(f"scene, protect_radius {r}: stats {s.tolist()}")
        assert int((v[~is_box] == REMOVED).sum()) == 0, "wall points removed, of 8 670"
        assert int((v[is_box] == REMOVED).sum()) == 96, "box points removed, of 96"
    h.close()


@pytest.mark.gpu
def test_stream_is_untouched_by_the_new_calls():
    """60 scans of the synthetic stream on two 2-slot handles with archive and grid; one of them calls the new functions every 20 scans"""
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(60)]
    opts = binding.occ_opts(origin=(-40.0, -40.0, -3.0), cell=(0.5, 0.5, 0.5), n=(160, 160, 12), min_range=1.0, max_range=35.0)
    rule = SR(protect_radius=1, keep_below=-1.0)

    def run(with_calls):
        h = binding.Handle(p, n_slots=2)
        h.replay_create(1, 60)
        for k, pts in enumerate(scans):
            h.replay_load(0, k, pts)
        h.replay_assign(0, 0, 0)
        h.replay_assign(1, 0, 9)
        h.map_enable(64, 1 << 20)
        h.occ_enable(opts)
        h.profile_enable(True)
        for first in (0, 20, 40):
            h.batch_run(first, 20, stages=7 | binding.REPLAY_BAG, sync=True)
            if with_calls:
                for s in range(2):
                    h.occ_mark(ALL, rule, s)
                    h.map_assemble_static(ALL | FID, 0.0, rule, s)
                    h.map_assemble_static(ALL, 0.4, None, s)
        names = list(h.profile_report())
        h.profile_enable(False)
        return h, names

    (a, names_a), (b, names_b) = run(False), run(True)
    new = ("occ_mark", "occ_offsets", "occ_emit")
    assert not [n for n in names_a if n in new], "a handle that never calls them launches none of the new kernels"
    assert all(n in names_b for n in new)
    for s in range(2):
        assert a.map_status(s)[0] >= 3
        pa, pb = a.batch_get_pose(s), b.batch_get_pose(s)
        assert pa[0] == pb[0], f"slot {s}: flags"
        for k in (1, 2):
            for key in ("t", "q"):
                assert_bit_equal(pa[k][key], pb[k][key], f"slot {s}: pose {k} {key}")
        for name in ("lm_state", "lm_info"):
            assert_bit_equal(a.debug_get(name, slot=s), b.debug_get(name, slot=s), f"slot {s}: {name}")
        assert_bit_equal(a.map_keyposes(s), b.map_keyposes(s), f"slot {s}: key poses")
        assert_bit_equal(a.map_assemble(ALL | FID, slot=s), b.map_assemble(ALL | FID, slot=s), f"slot {s}: archive")
        assert_bit_equal(a.map_assemble(ALL, 0.4, slot=s), b.map_assemble(ALL, 0.4, slot=s), f"slot {s}: filtered map")
    for h in (a, b):
        h.occ_integrate(slot=0)
        h.occ_integrate(slot=1)
    for ga, gb, name in zip(a.occ_get(), b.occ_get(), ("hits", "passes")):
        assert np.array_equal(ga, gb), f"the grid's {name}"
    # the stream's archive through the whole path on the handle that was left alone until now: leaf 0.4 by the one-workgroup VoxelGrid, then by
    # the multi-kernel one (ALEGO_GV_SMALL_MAX 0 sends every cloud there)
    for s in range(2):
        raw, v, st = _check(a, opts, f"stream, slot {s}", rule=rule, slot=s)
        print(f"stream, slot {s}: {raw.shape[0]} points, stats {st.tolist()}")
        assert st.sum() == raw.shape[0] > 4096
        kept = a.map_assemble(ALL, slot=s)[v != REMOVED]
        small, _ = a.map_assemble_static(ALL, 0.4, rule, s)
        assert_bit_equal(small, a.voxel_grid_large(kept, 0.4), f"stream, slot {s}: leaf 0.4")
    a.set_option("ALEGO_GV_SMALL_MAX", 0)
    for s in range(2):
        raw, v, _ = _check(a, opts, f"stream, slot {s}, multi-kernel VoxelGrid", rule=rule, slot=s)
        large, _ = a.map_assemble_static(ALL, 0.4, rule, s)
        assert_bit_equal(large, a.voxel_grid_large(a.map_assemble(ALL, slot=s)[v != REMOVED], 0.4), f"stream, slot {s}: leaf 0.4, multi-kernel")
        assert 0 < large.shape[0] < raw.shape[0]
    a.close(); b.close()


@pytest.mark.gpu
def test_replay_writes_the_static_map(tmp_path):
    exe = os.path.join(ROOT, "examples", "replay")
    r = subprocess.run([exe, "60", "--save-map", str(tmp_path), "--static", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("static: ")][0].split()
    assert line[1:12:2] == ["kept_occupied", "unknown", "outside", "below", "neighbour", "removed"] and line[13] == "of"
    printed, total = [int(line[i]) for i in (2, 4, 6, 8, 10, 12)], int(line[14])
    p = synth.default_params(16, 1800)
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    for k in range(60):
        h.scan_process(synth.scan(p, k), stages=7, stamp=0.1 * k)
    kp = h.map_keyposes()[:, :3].astype(np.float64)
    margin = np.array([30.0, 30.0, 3.0])
    origin = np.floor((kp.min(axis=0) - margin) / 0.5) * 0.5
    n = np.ceil((kp.max(axis=0) + margin - origin) / 0.5).astype(int)
    h.occ_enable(binding.occ_opts(origin, 0.5, n, 0.0, 30.0))
    h.occ_integrate()
    want, stats = h.map_assemble_static(ALL)
    assert stats.tolist() == printed and total == stats.sum() == h.map_assemble(ALL).shape[0]
    head = open(tmp_path / "static.pcd", "rb").read(600).decode("ascii", "replace")
    points = [int(ln.split()[1]) for ln in head.splitlines() if ln.startswith("POINTS ")]
    assert points == [want.shape[0]] and want.shape[0] == total - stats[REMOVED]
    h.close()
    # --static needs --save-map and excludes --occupancy: refused before any scan runs
    for args in (["--static", "0.5"], ["--save-map", str(tmp_path), "--static", "0.5", "--occupancy", "0.5", str(tmp_path)], ["--save-map", str(tmp_path), "--static", "-1"]):
        assert subprocess.run([exe, "2"] + args, capture_output=True, text=True, timeout=120).returncode == 2, args
