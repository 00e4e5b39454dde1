"""-m "not gpu": csrc/occ_math.h - the rule of the occupancy grid - on the host.

tests/occ_math/occ_math_check.cpp is built here with AddressSanitizer and UBSan as a program of its own (the header must be readable by a host
compiler without the HIP runtime): the invariants of the walk, sub-ranges from the closed form, the clip, the classes.

The host twins are then compared through the binding with tests/occ_ref.py, an exact rational traversal that shares no code with the library:
cell sequences on the issue's generator (rays near a tie left out, at most 1 %), the tie rule on constructed rays cell by cell, and the
accumulated counts and classes against numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import occ_ref as ref
from alego_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_occ_enable", "alego_occ_clear", "alego_occ_integrate", "alego_occ_get", "alego_occ_classify", "alego_occ_ray_host",
               "alego_occ_integrate_host", "alego_occ_classify_host"]
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8))   # the grid of the constructed rays


def test_math_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "occ_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "occ_math", "occ_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "occ_math ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_header_library_and_binding_have_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(binding.lib(), s) and s in binding.EXPORTS, s
    assert C.sizeof(binding.OccOpts) == 24 + 24 + 16 + 16 and C.sizeof(binding.OccRule) == 16
    m = re.search(r"enum \{ ALEGO_OCC_RAYS = 0, ALEGO_OCC_SHORT, ALEGO_OCC_TRUNCATED, ALEGO_OCC_CULLED, ALEGO_OCC_BAD, ALEGO_OCC_UPDATES, ALEGO_OCC_STATS \}", hdr)
    assert m and (binding.OCC_RAYS, binding.OCC_SHORT, binding.OCC_TRUNCATED, binding.OCC_CULLED, binding.OCC_BAD, binding.OCC_UPDATES, binding.OCC_STATS) == tuple(range(7))
    for name, v in (("SHORT", binding.OCC_SKIP_SHORT), ("CULLED", binding.OCC_SKIP_CULLED), ("BAD", binding.OCC_SKIP_BAD)):
        assert re.search(rf"ALEGO_OCC_SKIP_{name} = {v}\b", hdr) and v == getattr(ref, f"SKIP_{name}")


def _opts(grid, **kw):
    return binding.occ_opts(*grid, **kw)


def _twin(grid, o, e, **kw):
    return binding.occ_ray_host(_opts(grid, **kw), o, e)


def test_twin_gives_the_exact_traversal_on_the_generator():
    o, e, grid = ref.generator(3000, seed=1)
    left_out, cells_total = 0, 0
    for i in range(o.shape[0]):
        want, hit, near = ref.ray(*grid, o[i], e[i])
        if near:
            left_out += 1
            continue
        got, got_hit = _twin(grid, o[i], e[i])
        if isinstance(want, int):
            assert got == want, f"ray {i}: skip code"
            continue
        assert got_hit == hit and got.shape == want.shape and np.array_equal(got, want), f"ray {i}: cell sequence"
        cells_total += want.shape[0]
    print(f"{left_out} of {o.shape[0]} rays near a tie, {cells_total / o.shape[0]:.1f} cells per ray")
    assert left_out <= o.shape[0] // 100
    assert cells_total > 30 * o.shape[0]


def _seq(cells):
    return [tuple(int(v) for v in c) for c in cells]


def test_diagonal_through_cell_corners_steps_x_then_y_then_z():
    got, hit = _twin(UNIT, (0.5, 0.5, 0.5), (3.5, 3.5, 3.5))
    want = [(0, 0, 0)]
    for i in range(1, 4):
        want += [(i, i - 1, i - 1), (i, i, i - 1), (i, i, i)]
    assert _seq(got) == want and hit == 1
    assert _seq(ref.ray(*UNIT, (0.5, 0.5, 0.5), (3.5, 3.5, 3.5))[0]) == want
    # the same backwards, and a diagonal in y and z alone
    back, _ = _twin(UNIT, (3.5, 3.5, 3.5), (0.5, 0.5, 0.5))
    want_b = [(3, 3, 3)]
    for i in (2, 1, 0):
        want_b += [(i, i + 1, i + 1), (i, i, i + 1), (i, i, i)]
    assert _seq(back) == want_b
    yz, _ = _twin(UNIT, (0.5, 0.5, 0.5), (0.5, 2.5, 2.5))
    assert _seq(yz) == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 2, 1), (0, 2, 2)]


def test_ray_along_a_cell_face_stays_in_the_upper_cell():
    got, hit = _twin(UNIT, (0.5, 2.0, 0.5), (3.5, 2.0, 0.5))
    assert _seq(got) == [(0, 2, 0), (1, 2, 0), (2, 2, 0), (3, 2, 0)] and hit == 1


def test_start_on_a_boundary_in_both_directions():
    up, _ = _twin(UNIT, (2.0, 0.5, 0.5), (4.5, 0.5, 0.5))
    assert _seq(up) == [(2, 0, 0), (3, 0, 0), (4, 0, 0)]
    down, _ = _twin(UNIT, (2.0, 0.5, 0.5), (0.5, 0.5, 0.5))   # the boundary point belongs to cell 2: its first crossing lies at t = 0
    assert _seq(down) == [(2, 0, 0), (1, 0, 0), (0, 0, 0)]
    # ... with a second axis that crosses later
    both, _ = _twin(UNIT, (2.0, 0.5, 0.5), (0.5, 1.5, 0.5))
    assert _seq(both) == _seq(ref.ray(*UNIT, (2.0, 0.5, 0.5), (0.5, 1.5, 0.5))[0])


def test_zero_length_ray_and_start_cell_equal_to_end_cell():
    got, hit = _twin(UNIT, (1.25, 2.5, 3.75), (1.25, 2.5, 3.75))
    assert _seq(got) == [(1, 2, 3)] and hit == 1
    got, hit = _twin(UNIT, (1.25, 2.5, 3.75), (1.75, 2.25, 3.5))
    assert _seq(got) == [(1, 2, 3)] and hit == 1
    assert _twin(UNIT, (1.25, 2.5, 3.75), (1.25, 2.5, 3.75), min_range=0.5) == (binding.OCC_SKIP_SHORT, None)


def test_each_skip_code():
    assert _twin(UNIT, (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), min_range=1.5)[0] == binding.OCC_SKIP_SHORT
    assert isinstance(_twin(UNIT, (0.5, 0.5, 0.5), (2.0, 0.5, 0.5), min_range=1.5)[0], np.ndarray)   # len2 == min_range^2 is not short
    for o, e in (((-0.5, 1, 1), (-3.5, 2, 2)), ((1, 8.0, 1), (2, 11.5, 1)), ((1, 1, 9), (1, 1, 8.0))):   # both ends beyond one side (8.0 is cell 8)
        assert _twin(UNIT, o, e)[0] == binding.OCC_SKIP_CULLED, (o, e)
        assert ref.ray(*UNIT, o, e)[0] == ref.SKIP_CULLED
    assert isinstance(_twin(UNIT, (-0.5, 1, 1), (8.5, 1, 1))[0], np.ndarray)   # ends on both sides: cast
    for o, e in (((np.nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, np.inf, 1)), ((0, 0, 0), (1, 1, -np.inf)), ((0, 0, 0), (1.5e9, 1, 1)), ((-1.5e9, 0, 0), (1, 1, 1))):
        assert _twin(UNIT, o, e)[0] == binding.OCC_SKIP_BAD, (o, e)
        assert ref.ray(*UNIT, o, e)[0] == ref.SKIP_BAD
    # exactly 2^30 cells from the origin is still a ray (culled here: both ends below the grid); one f32 step further it is bad
    assert _twin(UNIT, (-2.0 ** 30, 0.5, 0.5), (-2.0 ** 30 + 128, 0.5, 0.5))[0] == binding.OCC_SKIP_CULLED
    assert _twin(UNIT, (-2.0 ** 30 - 128, 0.5, 0.5), (-2.0 ** 30 + 128, 0.5, 0.5))[0] == binding.OCC_SKIP_BAD


def test_truncation_at_max_range():
    o, e = (0.5, 0.5, 0.5), (3.5, 0.5, 0.5)
    got, hit = _twin(UNIT, o, e, max_range=3.0)    # len2 == max_range^2: not truncated
    assert _seq(got) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)] and hit == 1
    got, hit = _twin(UNIT, o, e, max_range=2.0)    # e <- (2.5, 0.5, 0.5), no hit
    assert _seq(got) == [(0, 0, 0), (1, 0, 0), (2, 0, 0)] and hit == 0
    got, hit = _twin(UNIT, o, e, max_range=2.5)    # e <- (3.0, 0.5, 0.5): on the boundary, the upper cell
    assert _seq(got) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)] and hit == 0
    want, want_hit, _ = ref.ray(*UNIT, (0.5, 0.5, 0.5), (5.25, 6.5, 3.125), max_range=4.0)
    got, hit = _twin(UNIT, (0.5, 0.5, 0.5), (5.25, 6.5, 3.125), max_range=4.0)
    assert np.array_equal(got, want) and hit == want_hit == 0


GRIDS = [((-20.0, -20.0, -2.0), (0.4, 0.4, 0.5), (100, 100, 8), {}),
         ((-3.0, -6.0, -0.75), (0.7, 0.4, 1.5), (17, 23, 1), dict(min_range=2.0, max_range=12.0)),
         ((2.0, 2.0, -1.0), (0.5, 0.5, 0.5), (1, 1, 1), {})]


@pytest.mark.parametrize("case", range(len(GRIDS)))
def test_integrate_and_classify_twins_against_numpy(case):
    origin, cell, n, kw = GRIDS[case]
    o, e, _ = ref.generator(300, seed=2 + case)
    o = o[np.arange(o.shape[0]) // 5 * 5]            # five rays per origin, as frames have them
    e[11] = np.nan; e[12] = e[13]                    # a bad ray, a doubled one
    want_h, want_p, want_s, near = ref.accumulate(origin, cell, n, zip(o, e), **kw)
    assert not near, "a generated ray lies near a tie: choose another seed"
    opts = _opts((origin, cell, n), **kw)
    origins = np.concatenate([o, np.zeros((o.shape[0], 1), np.float32)], axis=1)
    pts = np.concatenate([e, np.arange(o.shape[0], dtype=np.float32)[:, None]], axis=1)
    hits, passes, stats = binding.occ_integrate_host(opts, origins, pts)
    print(f"grid {case}: stats {stats.tolist()}, occupied cells {int((hits > 0).sum())}")
    assert np.array_equal(stats, want_s) and np.array_equal(hits, want_h) and np.array_equal(passes, want_p)
    assert stats[binding.OCC_UPDATES] == int(hits.sum(dtype=np.int64) + passes.sum(dtype=np.int64))
    # a second call adds to the same arrays
    binding.occ_integrate_host(opts, origins, pts, hits, passes, stats)
    assert np.array_equal(stats, 2 * want_s) and np.array_equal(hits, 2 * want_h) and np.array_equal(passes, 2 * want_p)
    for rule in (None, (1, 2, 1), (3, 1, 1), (0, 0, 0), (2, 1, 5)):
        mh, hw, pw = rule or (1, 2, 1)
        h64, p64 = hits.astype(np.int64), passes.astype(np.int64)
        want = np.where((h64 >= mh) & (h64 * hw >= p64 * pw), 100, np.where(p64 > 0, 0, -1)).astype(np.int8)
        assert np.array_equal(binding.occ_classify_host(opts, hits, passes, rule), want), rule
        col = np.where((want == 100).any(axis=0), 100, np.where((want == 0).any(axis=0), 0, -1)).astype(np.int8)
        assert np.array_equal(binding.occ_classify_host(opts, hits, passes, rule, collapse_z=True), col), rule


def test_classes_on_both_sides_of_each_comparison():
    opts = _opts(((0, 0, 0), 1.0, (3, 1, 2)))
    hits = np.array([[[2, 1, 2]], [[2, 1, 0]]], np.uint32)
    passes = np.array([[[0, 0, 4]], [[5, 1, 0]]], np.uint32)
    got = binding.occ_classify_host(opts, hits, passes, (2, 2, 1))
    assert got.tolist() == [[[100, -1, 100]], [[0, 0, -1]]]
    assert binding.occ_classify_host(opts, hits, passes, (2, 2, 1), collapse_z=True).tolist() == [[100, 0, 100]]


def test_every_refusal_of_the_options():
    L = binding.lib()
    o, e = np.zeros(3, np.float32), np.ones(3, np.float32)
    good = dict(origin=(0.0, 0.0, 0.0), cell=(1.0, 1.0, 1.0), n=(4, 4, 4), min_range=0.0, max_range=0.0)
    ray = lambda opts: L.alego_occ_ray_host(C.byref(opts), o.ctypes.data, e.ctypes.data, None, 0, None)
    assert ray(binding.occ_opts(**good)) > 0
    bad = [dict(cell=(0.0, 1, 1)), dict(cell=(1, -1.0, 1)), dict(cell=(1, 1, np.nan)), dict(cell=(np.inf, 1, 1)), dict(n=(0, 4, 4)), dict(n=(4, 4, -1)),
           dict(n=(65536, 32768, 1)), dict(n=(2048, 2048, 512)), dict(origin=(np.nan, 0, 0)), dict(origin=(0, -np.inf, 0)), dict(min_range=-1.0),
           dict(min_range=np.nan), dict(max_range=np.inf)]
    hits, passes, out = np.zeros(64, np.uint32), np.zeros(64, np.uint32), np.zeros(64, np.int8)
    for b in bad:
        opts = binding.occ_opts(**dict(good, **b))
        assert ray(opts) == binding.ERR_ARG, b
        assert L.alego_occ_integrate_host(C.byref(opts), None, None, 0, hits.ctypes.data, passes.ctypes.data, None) == binding.ERR_ARG, b
        assert L.alego_occ_classify_host(C.byref(opts), None, hits.ctypes.data, passes.ctypes.data, 0, out.ctypes.data) == binding.ERR_ARG, b
    assert ray(binding.occ_opts(**dict(good, n=(2147483647, 1, 1)))) > 0
    opts = binding.occ_opts(**good)
    for rule in ((-1, 2, 1), (1, -2, 1), (1, 2, -1)):
        r = binding.OccRule(*rule, 0)
        assert L.alego_occ_classify_host(C.byref(opts), C.byref(r), hits.ctypes.data, passes.ctypes.data, 0, out.ctypes.data) == binding.ERR_ARG, rule
    assert L.alego_occ_classify_host(C.byref(opts), None, hits.ctypes.data, passes.ctypes.data, 0, out.ctypes.data) == 0
    # a point whose intensity is no frame id: refused before anything is added
    kp = np.zeros((1, 4), np.float32)
    for w in (-1.0, np.nan):
        pts = np.array([[1, 1, 1, 0], [2, 2, 2, w]], np.float32)
        assert L.alego_occ_integrate_host(C.byref(opts), kp.ctypes.data, pts.ctypes.data, 2, hits.ctypes.data, passes.ctypes.data, None) == binding.ERR_ARG
    assert not hits.any() and not passes.any()
