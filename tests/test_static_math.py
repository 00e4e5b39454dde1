"""-m "not gpu": the static-map rule of csrc/occ_math.h on the host.

tests/static_math/static_check.cpp is built here with AddressSanitizer and UBSan as a program of its own and checks 10^4 random points against the
plain definition.  The host twin alego_occ_mark_host is then compared through the binding with tests/static_ref.py, which shares no code with the
library: on the end points of the occupancy generator's rays, on constructed points for every verdict, and on the scene of a wall that every key
pose sees and a box that each frame sees somewhere else."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import occ_ref
import static_ref as ref
from alego_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_occ_mark", "alego_map_assemble_static", "alego_occ_mark_host"]
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8))
RULES = (dict(), dict(protect_radius=1), dict(protect_radius=2), dict(keep_below=-0.1), dict(protect_radius=1, keep_below=0.05, occ=(2, 3, 1)))


def _rule(occ=(1, 2, 1), protect_radius=0, keep_below=None):
    return binding.static_rule(occ, protect_radius, keep_below)


def _both(grid, hits, passes, pts, sensor_z=None, **rule):
    """the twin's (verdicts, stats) after they were found equal to the reference's"""
    got_v, got_s = binding.occ_mark_host(binding.occ_opts(*grid), hits, passes, pts, _rule(**rule), sensor_z)
    want_v, want_s = ref.mark(*grid, hits, passes, pts, sensor_z, **rule)
    bad = np.nonzero(got_v != want_v)[0]
    assert bad.size == 0, f"{rule}: verdicts differ at {bad[:5].tolist()}: got {got_v[bad[:5]].tolist()} want {want_v[bad[:5]].tolist()}"
    assert np.array_equal(got_s, want_s) and got_s.sum() == len(pts) and np.array_equal(got_s, np.bincount(got_v, minlength=ref.VERDICTS))
    return got_v, got_s


def test_header_library_and_binding_have_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(binding.lib(), s) and s in binding.EXPORTS, s
    assert C.sizeof(binding.StaticRule) == 32
    assert re.search(r"enum \{ ALEGO_STATIC_OCCUPIED = 0, ALEGO_STATIC_UNKNOWN, ALEGO_STATIC_OUTSIDE, ALEGO_STATIC_BELOW, ALEGO_STATIC_NEIGHBOUR, ALEGO_STATIC_REMOVED, "
                     r"ALEGO_STATIC_VERDICTS \}", hdr)
    names = ("OCCUPIED", "UNKNOWN", "OUTSIDE", "BELOW", "NEIGHBOUR", "REMOVED", "VERDICTS")
    assert tuple(getattr(binding, "STATIC_" + n) for n in names) == tuple(getattr(ref, n) for n in names) == (0, 1, 2, 3, 4, 5, 6)


def test_rule_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "static_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "static_math", "static_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "static ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def generated():
    """the generator's 3 000 rays accumulated by the host twin of the integration, without ranges"""
    o, e, grid = occ_ref.generator(3000, seed=1)
    origins = np.concatenate([o, np.zeros((o.shape[0], 1), np.float32)], axis=1)
    pts = np.concatenate([e, np.arange(o.shape[0], dtype=np.float32)[:, None]], axis=1)
    hits, passes, _ = binding.occ_integrate_host(binding.occ_opts(*grid), origins, pts)
    return grid, hits, passes, e, (e[:, 2] - o[:, 2]).astype(np.float32)


@pytest.mark.parametrize("case", range(len(RULES)))
def test_generator_end_points_equal_the_reference(generated, case):
    grid, hits, passes, e, sz = generated
    v, stats = _both(grid, hits, passes, e, sz, **RULES[case])
    print(f"{RULES[case]}: stats {stats.tolist()}")
    assert stats[ref.OUTSIDE] > 100 and stats[ref.REMOVED] > 100
    if RULES[case].get("protect_radius"):
        assert stats[ref.NEIGHBOUR] > 0
    if "keep_below" in RULES[case]:
        assert stats[ref.BELOW] > 100
    if "occ" not in RULES[case]:
        # after an integration without ranges every point inside the grid lies in the cell its own ray hit: at min_hits 1 none is UNKNOWN
        assert stats[ref.UNKNOWN] == 0 and stats[ref.OCCUPIED] > 100
    else:
        assert stats[ref.UNKNOWN] > 0   # (min_hits 2: a cell hit once and never passed)


def test_unknown_is_reachable_with_max_range():
    opts = binding.occ_opts(*UNIT, max_range=2.0)
    origins = np.array([[0.5, 0.5, 0.5, 0]], np.float32)
    pts = np.array([[5.5, 0.5, 0.5, 0]], np.float32)   # truncated to (2.5, 0.5, 0.5): nobody passed cell 5
    hits, passes, stats = binding.occ_integrate_host(opts, origins, pts)
    assert stats[binding.OCC_TRUNCATED] == 1 and not hits.any()
    v, _ = _both(UNIT, hits, passes, np.array([[5.5, 0.5, 0.5], [2.5, 0.5, 0.5], [1.5, 0.5, 0.5]], np.float32))
    assert v.tolist() == [ref.UNKNOWN, ref.REMOVED, ref.REMOVED]


def _counts(n, cells):
    """(hits, passes) of a grid with the given {(x, y, z): (hits, passes)}"""
    hits, passes = np.zeros((n[2], n[1], n[0]), np.uint32), np.zeros((n[2], n[1], n[0]), np.uint32)
    for (x, y, z), (h, p) in cells.items():
        hits[z, y, x], passes[z, y, x] = h, p
    return hits, passes


def test_every_verdict_constructed():
    # products beyond 32 bits, on both sides of the comparison
    big = (1, 2147483647, 2147483647)
    hits, passes = _counts(UNIT[2], {(1, 1, 1): (4000000000, 4000000000), (2, 1, 1): (3999999999, 4000000000)})
    v, _ = _both(UNIT, hits, passes, np.array([[1.5, 1.5, 1.5], [2.5, 1.5, 1.5]], np.float32), occ=big)
    assert v.tolist() == [ref.OCCUPIED, ref.REMOVED]
    # min_hits 0: a cell nobody visited is occupied (0 >= 0); one pass without a hit frees it
    hits, passes = _counts(UNIT[2], {(3, 3, 3): (0, 1)})
    v, _ = _both(UNIT, hits, passes, np.array([[0.5, 0.5, 0.5], [3.5, 3.5, 3.5]], np.float32), occ=(0, 2, 1))
    assert v.tolist() == [ref.OCCUPIED, ref.REMOVED]
    v, _ = _both(UNIT, hits, passes, np.array([[0.5, 0.5, 0.5], [3.5, 3.5, 3.5]], np.float32))
    assert v.tolist() == [ref.UNKNOWN, ref.REMOVED]
    # a point on a cell boundary belongs to the upper cell; one exactly on the grid's far face is outside, one on the near face inside
    hits, passes = _counts(UNIT[2], {(2, 0, 0): (1, 0), (1, 0, 0): (0, 1), (0, 0, 0): (1, 0), (7, 7, 7): (1, 0)})
    pts = np.array([[2.0, 0.5, 0.5], [np.nextafter(np.float32(2.0), np.float32(0.0)), 0.5, 0.5], [8.0, 7.5, 7.5], [7.5, 8.0, 7.5], [7.5, 7.5, 8.0],
                    [np.nextafter(np.float32(8.0), np.float32(0.0)), 7.5, 7.5], [0.0, 0.0, 0.0], [-1e-30, 0.5, 0.5]], np.float32)
    v, _ = _both(UNIT, hits, passes, pts)
    assert v.tolist() == [ref.OCCUPIED, ref.REMOVED, ref.OUTSIDE, ref.OUTSIDE, ref.OUTSIDE, ref.OCCUPIED, ref.OCCUPIED, ref.OUTSIDE]
    # NaN / inf in each coordinate, a coordinate beyond 2^30 cells (and beyond an int32)
    pts = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1.5e9, 1, 1], [1, -3.0e9, 1], [1, 1, 3.0e38]], np.float32)
    v, stats = _both(UNIT, hits, passes, pts, protect_radius=2)
    assert stats[ref.OUTSIDE] == 6
    # OUTSIDE comes before BELOW, BELOW before the classes; keep_below equal to z keeps the point in the classes (kept only when <)
    below = np.nextafter(np.float32(-0.5), np.float32(-1.0))
    v, _ = _both(UNIT, hits, passes, np.array([[9.5, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], np.float32),
                 np.array([-3.0, -0.5, below, below], np.float32), keep_below=-0.5)
    assert v.tolist() == [ref.OUTSIDE, ref.REMOVED, ref.BELOW, ref.BELOW]
    # a 1 x 1 x 1 grid: every radius sees only the cell itself
    one = ((2.0, 2.0, -1.0), (0.5, 0.5, 0.5), (1, 1, 1))
    for cell_counts, want in (((1, 0), ref.OCCUPIED), ((0, 1), ref.REMOVED), ((0, 0), ref.UNKNOWN)):
        for r in (0, 1, 2):
            v, _ = _both(one, *_counts(one[2], {(0, 0, 0): cell_counts}), np.array([[2.25, 2.25, -0.75], [2.5, 2.25, -0.75]], np.float32), protect_radius=r)
            assert v.tolist() == [want, ref.OUTSIDE]


@pytest.mark.parametrize("n", [(4, 4, 4), (3, 1, 2), (1, 5, 1)])
def test_neighbourhood_is_clipped_at_every_face(n):
    """one occupied cell anywhere, a point in the middle of every cell (all passed once): NEIGHBOUR exactly within the Chebyshev radius; a read that
    left the grid on one axis would come back on another and see the occupied cell of a neighbouring row"""
    grid = ((-1.0, 0.5, 2.0), (0.5, 0.25, 1.0), n)
    xs = np.array([(x, y, z) for z in range(n[2]) for y in range(n[1]) for x in range(n[0])])
    pts = (np.array(grid[0]) + (xs + 0.5) * np.array(grid[1])).astype(np.float32)
    for occ_cell in xs:
        hits, passes = np.zeros((n[2], n[1], n[0]), np.uint32), np.ones((n[2], n[1], n[0]), np.uint32)
        hits[occ_cell[2], occ_cell[1], occ_cell[0]] = 5
        dist = np.abs(xs - occ_cell).max(axis=1)
        for r in (0, 1, 2):
            v, _ = _both(grid, hits, passes, pts, protect_radius=r)
            want = np.where(dist == 0, ref.OCCUPIED, np.where(dist <= r, ref.NEIGHBOUR, ref.REMOVED))
            assert np.array_equal(v, want), (occ_cell.tolist(), r)


def test_every_refusal():
    L = binding.lib()
    good = binding.occ_opts(*UNIT)
    hits, passes = np.zeros(512, np.uint32), np.zeros(512, np.uint32)
    pts, z, v, stats = np.ones((4, 4), np.float32), np.zeros(4, np.float32), np.full(4, 77, np.uint8), np.full(6, -1, np.int64)

    def call(opts=good, rule=None, h=hits, p=passes, q=pts, sz=z, n=4, out=v, st=stats):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.alego_occ_mark_host(None if opts is None else C.byref(opts), None if rule is None else C.byref(rule), ptr(h), ptr(p), ptr(q), ptr(sz), n, ptr(out), ptr(st))

    for kw in (dict(opts=None), dict(h=None), dict(p=None), dict(q=None), dict(out=None), dict(n=-1), dict(opts=binding.occ_opts((0, 0, 0), (0.0, 1, 1), (8, 8, 8))),
               dict(opts=binding.occ_opts((0, 0, 0), 1.0, (8, 0, 8))), dict(rule=_rule(occ=(-1, 2, 1))), dict(rule=_rule(occ=(1, -2, 1))), dict(rule=_rule(occ=(1, 2, -1))),
               dict(rule=_rule(protect_radius=-1)), dict(rule=_rule(protect_radius=3)), dict(rule=_rule(keep_below=np.nan)), dict(rule=_rule(keep_below=np.inf)),
               dict(rule=_rule(keep_below=0.0), sz=None)):
        assert call(**kw) == binding.ERR_ARG, kw
    assert (v == 77).all() and (stats == -1).all(), "a refused call writes nothing"
    unused = _rule()
    unused.keep_below = np.nan   # not read while use_keep_below is 0
    assert call(rule=unused, sz=None) == 0 and call(st=None) == 0 and call(rule=_rule(protect_radius=2, keep_below=1.0)) == 0
    assert call(q=None, out=None, sz=None, n=0) == 0 and stats.tolist() == [0] * 6
    assert call() == 0 and stats.tolist() == [0, 4, 0, 0, 0, 0]   # stats are set, not added to


# ---- the scene: a wall every key pose sees, a box each frame sees at another place (static_ref.scene) ----
def test_scene_the_box_goes_and_the_wall_stays():
    kp, pts, is_box = ref.scene()
    assert pts.shape[0] == 8766 and is_box.sum() == 96
    hits, passes, stats = binding.occ_integrate_host(binding.occ_opts(*ref.SCENE_GRID), kp, pts)
    assert stats[binding.OCC_RAYS] == 8766 and stats[binding.OCC_UPDATES] == 299128 and stats[1:5].sum() == 0
    for r in (0, 1):
        v, s = _both(ref.SCENE_GRID, hits, passes, pts, protect_radius=r)
        print(f"protect_radius {r}: stats {s.tolist()}")
        assert int((v[~is_box] == ref.REMOVED).sum()) == 0, "wall points removed, of 8 670"
        assert int((v[is_box] == ref.REMOVED).sum()) == 96, "box points removed, of 96"
        assert s[ref.NEIGHBOUR] == 0 and s[ref.OCCUPIED] == 8670   # no box point has an occupied neighbour at r = 1
