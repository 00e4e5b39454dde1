"""The occupancy grid of a key-frame archive (alego_occ_*) on the device.

Archives are built with alego_lm_add_keyframe from hand-made clouds.  In every case the device's hits, passes and counters are compared for
EXACT equality with the host twin alego_occ_integrate_host fed by alego_map_assemble(kinds | ALEGO_MAP_FRAME_ID, leaf 0) and alego_map_keyposes
of the same handle (the twin itself stands against an exact rational traversal in tests/test_occ_math.py).  Every comparison is repeated for
three piece lengths of occ_cast's work distribution: one lane per ray (0), pieces of 3 steps (every ray is cut, every piece seeks) and the default."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
PIECES = (0, 3, 32)
G0 = dict(origin=(-8.0, -8.0, -2.0), cell=(0.4, 0.4, 0.5), n=(40, 40, 8))   # 16 m x 16 m x 4 m around the sensors


def _err(h):
    return binding.lib().alego_last_error(h._h).decode()


def _cloud(rng, n, spread=(9.0, 9.0, 1.5)):
    """n points of the sensor frame, uniform in +/- spread: a part of the rays leaves G0"""
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


def _twin(h, opts, kinds=ALL, slot=0, first=0, n=-1, into=None):
    pts, kp = h.map_assemble(kinds | binding.MAP_FRAME_ID, 0.0, slot=slot), h.map_keyposes(slot)
    last = kp.shape[0] if n < 0 else first + n
    pts = pts[(pts[:, 3] >= first) & (pts[:, 3] < last)]
    return binding.occ_integrate_host(opts, kp, pts, *(into or ()))


def _same(got, want, tag):
    for name, g, w in zip(("hits", "passes", "stats"), got, want):
        assert np.array_equal(g, w), f"{tag}: {name} differ at {np.argwhere(np.asarray(g) != np.asarray(w))[:4].tolist()}: got {np.asarray(g)[np.asarray(g) != np.asarray(w)][:4]} want {np.asarray(w)[np.asarray(g) != np.asarray(w)][:4]}"


def _check(h, opts, tag, kinds=ALL, slot=0, first=0, n=-1):
    """clear + integrate for every piece length against the twin; returns the twin's (hits, passes, stats)"""
    want = _twin(h, opts, kinds, slot, first, n)
    for piece in PIECES:
        h.debug_occ_piece(piece)
        h.occ_clear()
        stats = h.occ_integrate(kinds, first, n, slot)
        _same((*h.occ_get(), stats), want, f"{tag}, piece {piece}")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 256, 257])
def test_one_frame(params_a, n_points):
    rng = np.random.default_rng(100 + n_points)
    opts = binding.occ_opts(**G0)
    h = _handle(params_a, opts, {0: [_frame(rng, (0.3, -0.2, 0.1, 0.02, -0.03, 0.4), 0, n_points, 0)]})
    hits, passes, stats = _check(h, opts, f"{n_points} points")
    assert stats[binding.OCC_RAYS] == n_points and stats[binding.OCC_UPDATES] == int(hits.sum()) + int(passes.sum()) > 0
    h.close()


@pytest.fixture(scope="module")
def three_frames(params_a):
    """3 frames with rotated poses; each has one empty cloud, frame 1 straddles a chunk of occ_cast (300 selected points)"""
    rng = np.random.default_rng(7)
    frames = [_frame(rng, (0.5, 0.25, 0.0, 0.05, -0.1, 0.7), 0, 90, 40), _frame(rng, (-2.0, 1.5, 0.3, -0.2, 0.1, -2.5), 130, 0, 170),
              _frame(rng, (3.0, -3.5, -0.4, 0.3, 0.25, 3.0), 60, 45, 0)]
    opts = binding.occ_opts(**G0)
    h = _handle(params_a, opts, {0: frames})
    yield h, opts
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", range(1, 8))
def test_each_kinds_mask(three_frames, kinds):
    h, opts = three_frames
    _, _, stats = _check(h, opts, f"kinds {kinds}", kinds=kinds)
    want = sum(n for bit, n in ((binding.MAP_CORNER, 0 + 130 + 60), (binding.MAP_SURF, 90 + 0 + 45), (binding.MAP_OUTLIER, 40 + 170 + 0)) if kinds & bit)
    assert stats[binding.OCC_RAYS] == want


@pytest.mark.gpu
def test_frame_ranges_and_accumulation(three_frames):
    h, opts = three_frames
    for first, n in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (1, -1), (0, -1), (0, 3), (3, 0), (3, -1), (0, 0)):
        _, _, stats = _check(h, opts, f"frames {first} + {n}", first=first, n=n)
        assert (stats[binding.OCC_RAYS] == 0) == (n == 0 or first == 3)
    # two calls add up to one call, whatever the kinds and ranges they split the work by
    whole = _twin(h, opts)
    h.debug_occ_piece(32)
    for parts in (((ALL, 0, 1), (ALL, 1, -1)), ((binding.MAP_SURF, 0, -1), (binding.MAP_CORNER | binding.MAP_OUTLIER, 0, -1))):
        h.occ_clear()
        stats = sum(h.occ_integrate(k, f, n) for k, f, n in parts)
        _same((*h.occ_get(), stats), whole, f"in two calls {parts}")
    # ... a third on top doubles nothing but its own share; clear starts over
    extra = _twin(h, opts, binding.MAP_OUTLIER, first=1, n=1, into=tuple(a.copy() for a in whole))
    stats = stats + h.occ_integrate(binding.MAP_OUTLIER, 1, 1)
    _same((*h.occ_get(), stats), extra, "a third call on top")
    h.occ_clear()
    assert not h.occ_get()[0].any() and not h.occ_get()[1].any()
    stats = h.occ_integrate()
    _same((*h.occ_get(), stats), whole, "clear, then integrate")


@pytest.mark.gpu
def test_classify_flat_and_collapsed(three_frames):
    h, opts = three_frames
    h.occ_clear()
    for _ in range(3):   # three times the archive: counts that tell the rules apart
        h.occ_integrate()
    hits, passes = h.occ_get()
    seen = set()
    for rule in (None, (1, 2, 1), (4, 1, 1), (0, 0, 0), (3, 1, 2), (1, 1, 30)):
        for collapse in (False, True):
            got = h.occ_classify(rule, collapse)
            assert np.array_equal(got, binding.occ_classify_host(opts, hits, passes, rule, collapse)), (rule, collapse)
            seen |= set(np.unique(got).tolist())
    assert seen == {-1, 0, 100}
    assert np.array_equal(h.occ_classify(), h.occ_classify((1, 2, 1)))


@pytest.mark.gpu
def test_thousand_identical_rays(params_a):
    """every cell on the ray holds exactly 1 000: any aggregation or lost-update fault shows"""
    opts = binding.occ_opts(**G0)
    surf = np.tile(np.array([[6.3, 4.1, 1.2, 0.5]], np.float32), (1000, 1))
    h = _handle(params_a, opts, {0: [dict(pose=np.array([-1.1, 0.2, -0.3, 0, 0, 0], np.float32), corner=np.zeros((0, 4), np.float32), surf=surf, outlier=np.zeros((0, 4), np.float32))]})
    hits, passes, stats = _check(h, opts, "1000 identical rays")
    cells, hit = binding.occ_ray_host(opts, (-1.1, 0.2, -0.3), h.map_assemble(binding.MAP_SURF)[0, :3])
    assert hit == 1 and cells.shape[0] > 20
    want_p, want_h = np.zeros_like(passes), np.zeros_like(hits)
    want_p[cells[:-1, 2], cells[:-1, 1], cells[:-1, 0]] = 1000
    want_h[cells[-1, 2], cells[-1, 1], cells[-1, 0]] = 1000
    assert np.array_equal(passes, want_p) and np.array_equal(hits, want_h) and stats[binding.OCC_UPDATES] == 1000 * cells.shape[0]
    h.close()


@pytest.mark.gpu
def test_long_rays_and_one_cell_rays(params_a):
    """the edges of any splitting: one ray through more than 1 000 cells alone, then a frame that mixes such rays with rays of one cell"""
    opts = binding.occ_opts(origin=(-30.0, -1.0, -1.0), cell=(0.05, 0.05, 0.5), n=(1200, 40, 4))
    none = np.zeros((0, 4), np.float32)
    long_ray = np.array([[57.9, 0.83, 0.4, 0]], np.float32)
    rng = np.random.default_rng(3)
    mixed = np.concatenate([np.concatenate([rng.uniform(50, 58, (40, 1)), rng.uniform(-0.9, 0.9, (40, 1)), rng.uniform(-0.9, 0.9, (40, 1)), np.zeros((40, 1))], axis=1),
                            np.concatenate([rng.uniform(-0.004, 0.004, (160, 3)), np.zeros((160, 1))], axis=1)]).astype(np.float32)
    mixed = mixed[rng.permutation(mixed.shape[0])]
    pose = np.array([-29.012, 0.012, 0.26, 0, 0, 0], np.float32)
    h = _handle(params_a, opts, {0: [dict(pose=pose, corner=none, surf=long_ray, outlier=none), dict(pose=pose, corner=none, surf=mixed, outlier=none)]})
    _, _, stats = _check(h, opts, "one long ray", first=0, n=1)
    assert stats[binding.OCC_UPDATES] > 1000 and stats[binding.OCC_RAYS] == 1
    hits, _, stats = _check(h, opts, "long and one-cell rays mixed", first=1, n=1)
    assert stats[binding.OCC_UPDATES] > 40 * 1000 and hits.max() >= 100   # (the one-cell rays end where they start)
    _check(h, opts, "both frames")
    h.close()


GRIDS = {
    "one_cell": dict(origin=(-0.5, -0.5, -0.5), cell=(1.5, 1.5, 1.0), n=(1, 1, 1)),
    "one_cell_far": dict(origin=(4.0, 2.0, -0.5), cell=(2.0, 2.0, 1.0), n=(1, 1, 1)),
    "excludes_the_sensor": dict(origin=(2.5, -6.0, -1.0), cell=(0.3, 0.5, 0.4), n=(20, 24, 5)),
    "every_ray_misses": dict(origin=(40.0, 40.0, 5.0), cell=(0.4, 0.4, 0.4), n=(10, 10, 10)),
    "one_layer_above_the_ground": dict(origin=(-8.0, -8.0, -0.4), cell=(0.4, 0.4, 1.4), n=(40, 40, 1)),
    "min_and_max_range": dict(origin=(-8.0, -8.0, -2.0), cell=(0.4, 0.4, 0.5), n=(40, 40, 8), min_range=3.0, max_range=7.0),
    "odd_cells": dict(origin=(-7.7, -8.3, -1.9), cell=(0.37, 0.53, 0.71), n=(43, 31, 5), max_range=9.5),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grids(params_a, name):
    rng = np.random.default_rng(11)
    opts = binding.occ_opts(**GRIDS[name])
    frames = [_frame(rng, (0.2, 0.1, 0.0, 0.0, 0.0, 0.3), 50, 200, 50), _frame(rng, (1.0, -0.5, 0.1, 0.1, -0.05, -1.0), 40, 120, 30)]
    ground = _cloud(rng, 150)
    ground[:, 2] = -1.2 + rng.uniform(-0.05, 0.05, 150).astype(np.float32)   # ground returns, below the one-layer grid
    frames[0]["outlier"] = np.concatenate([frames[0]["outlier"], ground])
    h = _handle(params_a, opts, {0: frames})
    hits, passes, stats = _check(h, opts, name)
    print(f"{name}: stats {stats.tolist()}")
    if name == "every_ray_misses":
        assert stats[binding.OCC_CULLED] == stats[binding.OCC_RAYS] and stats[binding.OCC_UPDATES] == 0 and not hits.any() and not passes.any()
    if name == "one_cell":
        assert hits[0, 0, 0] > 0 and passes[0, 0, 0] > 0
    if name == "excludes_the_sensor":
        assert stats[binding.OCC_CULLED] > 0 and stats[binding.OCC_UPDATES] > 0
    if name == "one_layer_above_the_ground":
        pts = h.map_assemble(ALL)
        assert hits.sum() < (pts[:, 2] >= -0.4).sum() + 1 and hits.sum() > 0 and (pts[:, 2] < -0.4).sum() >= 150
    if name == "min_and_max_range":
        assert stats[binding.OCC_SHORT] > 0 and stats[binding.OCC_TRUNCATED] > 0
    assert int(hits.sum()) == _hits_inside(h, opts)
    h.close()


def _hits_inside(h, opts):
    """rays that are cast untruncated and end inside the grid: each leaves one hit"""
    pts, kp = h.map_assemble(ALL | binding.MAP_FRAME_ID), h.map_keyposes()
    count = 0
    for p in pts:
        cells, hit = binding.occ_ray_host(opts, kp[int(p[3]), :3], p[:3])
        if hit == 1 and np.all((cells[-1] >= 0) & (cells[-1] < np.array(opts.n[:]))):
            count += 1
    return count


@pytest.mark.gpu
def test_bad_points_are_counted(params_a):
    opts = binding.occ_opts(**G0)
    rng = np.random.default_rng(5)
    fr = _frame(rng, (0, 0, 0, 0, 0, 0), 0, 70, 0)
    fr["surf"][3, 0] = np.nan; fr["surf"][17, 2] = np.inf; fr["surf"][40, 1] = 3.0e9
    h = _handle(params_a, opts, {0: [fr]})
    _, _, stats = _check(h, opts, "non-finite and far points")
    assert stats[binding.OCC_BAD] == 3
    h.close()


@pytest.mark.gpu
def test_moved_key_pose(three_frames):
    h, opts = three_frames
    before = _check(h, opts, "before the move")
    old = np.concatenate([h.map_get_keyframe(1)["pose"]])
    h.map_set_keyposes(1, np.array([[1.5, 2.5, -0.2, 0.1, 0.2, 1.0]], np.float32))
    after = _check(h, opts, "after alego_map_set_keyposes")   # (the twin reads the new assembly)
    assert not np.array_equal(before[0], after[0])
    h.map_set_keyposes(1, old[None, :])
    _same(_check(h, opts, "moved back"), before, "moved back")


@pytest.mark.gpu
def test_slots(params_a, monkeypatch):
    """two slots into one grid give the sum; slot 1 of a 3-slot handle (two stream groups) gives what a one-slot replica gives"""
    rng = np.random.default_rng(21)
    fa = [_frame(rng, (0.5, 0.5, 0, 0, 0, 0.5), 30, 100, 20), _frame(rng, (-1, 1, 0.2, 0.1, 0, -0.5), 10, 80, 40)]
    fb = [_frame(rng, (2.0, -2.0, 0.1, 0, 0.1, 2.0), 64, 64, 64)]
    opts = binding.occ_opts(**G0)
    monkeypatch.setenv("ALEGO_STREAM_GROUPS", "2")
    h = _handle(params_a, opts, {1: fa, 2: fb}, n_slots=3)
    monkeypatch.delenv("ALEGO_STREAM_GROUPS")
    assert h.stream_groups()[0] == 2
    r = _handle(params_a, opts, {0: fa})
    want1 = _check(r, opts, "replica")
    _same(_check(h, opts, "slot 1 of 3", slot=1), want1, "slot 1 against the replica")
    want2 = _check(h, opts, "slot 2 of 3", slot=2)
    assert _check(h, opts, "the empty slot 0", slot=0)[2][binding.OCC_RAYS] == 0
    h.occ_clear()
    stats = h.occ_integrate(slot=1) + h.occ_integrate(slot=2)
    _same((*h.occ_get(), stats), tuple(a + b for a, b in zip(want1, want2)), "two slots into one grid")
    h.close(); r.close()


@pytest.mark.gpu
def test_every_refusal(params_a):
    L = binding.lib()
    rng = np.random.default_rng(2)
    opts = binding.occ_opts(**G0)
    stats, cells = np.zeros(binding.OCC_STATS, np.int64), np.zeros(40 * 40 * 8, np.uint32)
    out = np.zeros(40 * 40 * 8, np.int8)

    def calls(h):
        return (L.alego_occ_clear(h._h), L.alego_occ_integrate(h._h, 0, 0, -1, ALL, stats.ctypes.data), L.alego_occ_get(h._h, cells.ctypes.data, None),
                L.alego_occ_classify(h._h, None, 0, out.ctypes.data))

    h = binding.Handle(params_a, n_slots=2)
    assert L.alego_occ_enable(h._h, C.byref(opts)) == binding.ERR_ARG and "archive is off" in _err(h)   # archive off
    assert calls(h) == (binding.ERR_ARG,) * 4
    h.map_enable(8, 4096)
    assert calls(h) == (binding.ERR_ARG,) * 4 and "alego_occ_enable" in _err(h)                          # before enable
    assert L.alego_occ_enable(h._h, None) == binding.ERR_ARG and L.alego_occ_enable(None, C.byref(opts)) == binding.ERR_ARG
    good = dict(G0, min_range=0.0, max_range=0.0)
    for b in (dict(cell=(0.0, 1, 1)), dict(cell=(1, -1.0, 1)), dict(cell=(1, 1, np.nan)), dict(cell=(np.inf, 1, 1)), dict(n=(0, 4, 4)), dict(n=(4, 4, -1)),
              dict(n=(65536, 32768, 1)), dict(n=(2048, 2048, 512)), dict(origin=(np.nan, 0, 0)), dict(origin=(0, -np.inf, 0)), dict(min_range=-1.0),
              dict(min_range=np.nan), dict(max_range=np.inf)):
        assert L.alego_occ_enable(h._h, C.byref(binding.occ_opts(**dict(good, **b)))) == binding.ERR_ARG and "occ_enable" in _err(h), b
    assert calls(h) == (binding.ERR_ARG,) * 4                                                                    # a refused enable enables nothing
    for fr in (_frame(rng, (0, 0, 0, 0, 0, 0), 5, 5, 5), _frame(rng, (1, 0, 0, 0, 0, 0), 5, 5, 5)):
        h.lm_add_keyframe(fr["pose"], fr["corner"], fr["surf"], fr["outlier"])
    h.occ_enable(opts)                                                                                           # (after key frames exist: allowed)
    assert L.alego_occ_enable(h._h, C.byref(opts)) == binding.ERR_ARG and "already enabled" in _err(h)    # a second enable
    assert calls(h) == (0,) * 4
    integ = lambda slot, first, n, kinds: L.alego_occ_integrate(h._h, slot, first, n, kinds, stats.ctypes.data)
    for slot, first, n, kinds in ((0, -1, 1, ALL), (0, 0, 3, ALL), (0, 3, -1, ALL), (0, 2, 1, ALL), (0, 0, -2, ALL), (1, 0, 1, ALL), (0, 0, -1, 0), (0, 0, -1, 8),
                                  (2, 0, -1, ALL), (-1, 0, -1, ALL)):
        assert integ(slot, first, n, kinds) == binding.ERR_ARG and _err(h), (slot, first, n, kinds)
    assert integ(0, 0, 2, ALL) == 0 and integ(0, 2, 0, ALL) == 0 and integ(1, 0, 0, ALL) == 0 and integ(0, 0, -1, ALL | 8) == 0
    assert L.alego_occ_integrate(h._h, 0, 0, -1, ALL, None) == 0                                                 # stats may be NULL
    assert L.alego_occ_get(h._h, None, None) == 0
    for rule in ((-1, 2, 1), (1, -2, 1), (1, 2, -1)):
        assert L.alego_occ_classify(h._h, C.byref(binding.OccRule(*rule, 0)), 0, out.ctypes.data) == binding.ERR_ARG and "negative" in _err(h), rule
    assert L.alego_occ_classify(h._h, None, 0, None) == binding.ERR_ARG
    h.close()


@pytest.mark.gpu
def test_localising_handle_is_refused(params_a):
    rng = np.random.default_rng(4)
    fr = _frame(rng, (0, 0, 0, 0, 0, 0), 20, 60, 20)
    h = binding.Handle(params_a)
    h.loc_enable([(fr["pose"], fr["corner"], fr["surf"], fr["outlier"])])
    assert binding.lib().alego_occ_enable(h._h, C.byref(binding.occ_opts(**G0))) == binding.ERR_ARG and "localising" in _err(h)
    h.close()


@pytest.mark.gpu
def test_stream_is_untouched_and_grid_equals_twin():
    """60 scans of the synthetic stream on two 2-slot handles with the archive on; one has the grid enabled from the start and integrates at the end"""
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(60)]
    opts = binding.occ_opts(origin=(-40.0, -40.0, -3.0), cell=(0.5, 0.5, 0.5), n=(160, 160, 12), min_range=1.0, max_range=35.0)

    def run(with_grid):
        h = binding.Handle(p, n_slots=2)
        h.replay_create(1, 60)
        for k, pts in enumerate(scans):
            h.replay_load(0, k, pts)
        h.replay_assign(0, 0, 0)
        h.replay_assign(1, 0, 9)
        h.map_enable(64, 1 << 20)
        if with_grid:
            h.occ_enable(opts)
        h.profile_enable(True)
        h.batch_run(0, 60, stages=7 | binding.REPLAY_BAG, sync=True)
        names = list(h.profile_report())
        h.profile_enable(False)
        return h, names

    (a, names_a), (b, names_b) = run(False), run(True)
    assert not [n for n in names_a + names_b if n.startswith("occ_")], "an enabled grid launches nothing on the per-scan path"
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
        assert_bit_equal(a.map_assemble(ALL | binding.MAP_FRAME_ID, slot=s), b.map_assemble(ALL | binding.MAP_FRAME_ID, slot=s), f"slot {s}: archive")
    want = _twin(b, opts, slot=0)
    want = _twin(b, opts, slot=1, into=want)
    stats = b.occ_integrate(slot=0) + b.occ_integrate(slot=1)
    _same((*b.occ_get(), stats), want, "the stream's grid")
    print(f"stream: stats {stats.tolist()}")
    assert stats[binding.OCC_UPDATES] > 100000 and stats[binding.OCC_SHORT] + stats[binding.OCC_TRUNCATED] > 0
    assert "occ_cast" not in a.profile_report()
    a.close(); b.close()


@pytest.mark.gpu
def test_replay_writes_the_classified_grid(tmp_path):
    exe = os.path.join(ROOT, "examples", "replay")
    r = subprocess.run([exe, "60", "--occupancy", "0.5", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("occupancy: ")][0].split()
    f = dict(origin=[float(v) for v in line[2:5]], cell=[float(v) for v in line[6:9]], n=[int(v) for v in line[10:13]], max_range=float(line[14]))
    stats_line = [int(line[i]) for i in (16, 18, 20, 22, 24, 26)]
    assert f["cell"][:2] == [0.5, 0.5] and f["n"][2] == 1 and f["max_range"] == 30.0
    p = synth.default_params(16, 1800)
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    for k in range(60):
        h.scan_process(synth.scan(p, k), stages=7, stamp=0.1 * k)
    kp = h.map_keyposes()
    lo, hi = kp[:, :3].astype(np.float64).min(axis=0), kp[:, :3].astype(np.float64).max(axis=0)
    for a in range(2):   # the grid covers the key poses' bounding box plus max_range, on multiples of the cell
        assert f["origin"][a] <= lo[a] - 30.0 < f["origin"][a] + 0.5 and f["origin"][a] + 0.5 * f["n"][a] >= hi[a] + 30.0 > f["origin"][a] + 0.5 * (f["n"][a] - 1)
    assert f["origin"][2] == lo[2] - 0.5 and f["origin"][2] + f["cell"][2] == pytest.approx(hi[2] + 1.0, abs=1e-12)
    opts = binding.occ_opts(f["origin"], f["cell"], f["n"], 0.0, f["max_range"])
    h.occ_enable(opts)
    stats = h.occ_integrate()
    assert stats.tolist() == stats_line
    want = h.occ_classify(collapse_z=True)
    raw = open(tmp_path / "occupancy.pgm", "rb").read()
    head = f"P5\n{f['n'][0]} {f['n'][1]}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + f["n"][0] * f["n"][1]
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(f["n"][1], f["n"][0])
    assert set(np.unique(img).tolist()) == {0, 205, 254}
    assert np.array_equal(img[::-1], np.where(want == 100, 0, np.where(want == 0, 254, 205)).astype(np.uint8))
    yaml = dict(ln.split(": ", 1) for ln in open(tmp_path / "occupancy.yaml").read().splitlines())
    assert yaml["image"] == "occupancy.pgm" and float(yaml["resolution"]) == 0.5 and [float(v) for v in yaml["origin"].strip("[]").split(",")] == f["origin"][:2] + [0.0]
    h.close()
