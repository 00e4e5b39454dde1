"""-m "not gpu": the clearance field and the cost map of csrc/edt_math.h on the host.

tests/edt_math/edt_check.cpp is built here with AddressSanitizer and UBSan as a program of its own: the envelope of 10^4 random lines against the
O(n^2) definition, the sign of every sep numerator, the domain rule.  The host twins alego_occ_distance_host, alego_occ_cost_table_host and
alego_occ_costmap_host are then compared through the binding with tests/edt_ref.py, which shares no code with the library.  Every comparison is over
all cells, for equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edt_ref as ref
from alego_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_occ_set", "alego_occ_distance", "alego_occ_costmap", "alego_occ_distance_host", "alego_occ_cost_table_host", "alego_occ_costmap_host"]
TABLES = ((0.2, 0.35, 2.0, 3.0), (0.05, 0.33, 1.5, 10.0), (0.4, 0.5, 3.0, 1.0), (0.1, 0.0, 1.0, 5.0))   # (s, inscribed, radius, scaling)


def _both(cls, unknown_is_obstacle=False, max_cells=0):
    """the twin's (d2, stats) after they were found equal to the reference's"""
    got, gs = binding.occ_distance_host(cls, unknown_is_obstacle, max_cells)
    want, ws = ref.distance(cls, unknown_is_obstacle, max_cells)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"d2 differs at {bad[:5].tolist()}: got {got[got != want][:5].tolist()} want {want[got != want][:5].tolist()}"
    assert gs.tolist() == ws.tolist(), (gs.tolist(), ws.tolist())
    return got, gs


def _random(rng, shape, density):
    """classes of `shape`: sources at `density` (a float), exactly one ("one"), none (0) or all (1); the rest free or unknown"""
    cls = rng.choice(np.array([0, -1], np.int8), size=shape)
    if density == "one":
        cls[tuple(int(rng.integers(n)) for n in shape)] = 100
    else:
        cls[rng.random(shape) < density] = 100
    return cls


def test_header_library_and_binding_have_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(binding.lib(), s) and s in binding.EXPORTS, s
    assert C.sizeof(binding.OccDistOpts) == 16 and C.sizeof(binding.OccInflation) == 32
    assert re.search(r"#define ALEGO_OCC_FAR 0xFFFFFFFFu", hdr) and binding.OCC_FAR == ref.FAR == 0xFFFFFFFF
    assert re.search(r"enum \{ ALEGO_EDT_SOURCES = 0, ALEGO_EDT_FAR_CELLS, ALEGO_EDT_MAX_D2, ALEGO_EDT_STATS \}", hdr)
    assert (binding.EDT_SOURCES, binding.EDT_FAR_CELLS, binding.EDT_MAX_D2, binding.EDT_STATS) == (0, 1, 2, 3)
    assert re.search(r"typedef struct alego_occ_dist_opts \{ int32_t collapse_z, unknown_is_obstacle, max_cells, pad; \}", hdr)
    assert re.search(r"typedef struct alego_occ_inflation \{ double inscribed_radius, inflation_radius, cost_scaling; int32_t inflate_unknown, pad; \}", hdr)
    for name in ("occ_set", "occ_distance", "occ_costmap"):
        assert hasattr(binding.Handle, name), name


def test_rule_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "edt_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "edt_math", "edt_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "edt ok" in r.stdout and "none negative" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("density", [0.0, "one", 0.005, 0.05, 0.5, 1.0])
def test_random_grids_equal_brute_force(density):
    rng = np.random.default_rng(31 if density == "one" else int(1000 * density) + 7)
    shapes = [tuple(int(v) for v in rng.integers(1, 13, 3)) for _ in range(12)] + [(1, 1, 1), (12, 12, 12), (5, 29, 37)]
    for shape in shapes:
        cls = _random(rng, shape, density)
        d2, stats = _both(cls)
        if density == 0.0:
            assert (d2 == ref.FAR).all() and stats.tolist() == [0, cls.size, -1]
        if density == 1.0:
            assert not d2.any() and stats.tolist() == [cls.size, 0, 0]
        if density == "one":
            assert stats[0] == 1 and stats[1] == 0


def test_constructed_cases():
    n = (6, 7, 9)   # (n2, n1, n0)
    for corner in np.ndindex(2, 2, 2):   # a source in each corner
        cls = np.zeros(n, np.int8)
        at = tuple(c * (m - 1) for c, m in zip(corner, n))
        cls[at] = 100
        d2, stats = _both(cls)
        far = tuple(m - 1 - a for a, m in zip(at, n))
        assert d2[at] == 0 and d2[far] == 5 * 5 + 6 * 6 + 8 * 8 == stats[2]
    cls = np.zeros(n, np.int8)   # two equidistant sources: the cells between see both at the same distance
    cls[3, 3, 2] = cls[3, 3, 6] = 100
    d2, _ = _both(cls)
    assert d2[3, 3, 4] == 4 and d2[3, 3, 3] == d2[3, 3, 5] == 1 and d2[0, 3, 4] == 9 + 4
    for axis in range(3):   # a full plane across each axis
        cls = np.full(n, -1, np.int8)
        idx = [slice(None)] * 3
        idx[axis] = 2
        cls[tuple(idx)] = 100
        d2, stats = _both(cls)
        want = (np.arange(n[axis]) - 2) ** 2
        assert np.array_equal(d2, np.broadcast_to(want.reshape([-1 if a == axis else 1 for a in range(3)]), n))
        assert stats.tolist() == [cls.size // n[axis], 0, int(want.max())]
    for axis in range(3):   # a grid that is a single line along each axis in turn
        shape = [1, 1, 1]
        shape[axis] = 70
        cls = np.zeros(shape, np.int8)
        cls.reshape(-1)[[3, 40, 41]] = 100
        d2, _ = _both(cls)
        assert d2.reshape(-1)[[0, 21, 22, 69]].tolist() == [9, 18 * 18, 18 * 18, 28 * 28]
    for c, want in ((100, 0), (0, ref.FAR), (-1, ref.FAR)):   # 1 x 1 x 1 with and without a source
        d2, stats = _both(np.full((1, 1, 1), c, np.int8))
        assert d2.item() == want and stats.tolist() == ([1, 0, 0] if c == 100 else [0, 1, -1])
    d2, stats = _both(np.full((1, 1, 1), -1, np.int8), unknown_is_obstacle=True)
    assert d2.item() == 0 and stats.tolist() == [1, 0, 0]


def test_caps_unknown_and_collapsed():
    rng = np.random.default_rng(5)
    cls = _random(rng, (5, 29, 37), 0.005)
    free, stats = _both(cls)
    no_cut = int(np.ceil(np.sqrt(stats[2])))   # the value at which nothing is cut
    for cap in (1, 3, no_cut):
        d2, s = _both(cls, max_cells=cap)
        assert ((d2 == ref.FAR) == (free > cap * cap)).all() and np.array_equal(d2[d2 != ref.FAR], free[free <= cap * cap])
        assert (s[1] == 0) == (cap == no_cut)
    assert no_cut > 3 and _both(cls, max_cells=no_cut - 1)[1][1] > 0
    unk, s = _both(cls, unknown_is_obstacle=True)
    assert s[0] == int((cls != 0).sum()) and (unk <= free).all() and (unk < free).any()
    for cap in (1, 3):
        _both(cls, unknown_is_obstacle=True, max_cells=cap)
    # a collapsed array is a grid of one layer: (n1, n0) and (1, n1, n0) give the same
    flat = _random(rng, (29, 37), 0.01)
    a, sa = _both(flat)
    b, sb = _both(flat[None])
    assert np.array_equal(a, b[0]) and sa.tolist() == sb.tolist()
    line, _ = _both(flat[4])
    assert line.shape == (37,)


def test_every_refusal():
    L = binding.lib()
    cls, d2, stats = np.zeros(64, np.int8), np.full(64, 77, np.uint32), np.full(3, -5, np.int64)

    def dist(c=cls, n=(4, 4, 4), uio=0, cap=0, out=d2, st=stats):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.alego_occ_distance_host(ptr(c), None if n is None else (C.c_int32 * 3)(*n), uio, cap, ptr(out), ptr(st))

    for kw in (dict(c=None), dict(n=None), dict(out=None, st=None), dict(n=(0, 4, 4)), dict(n=(4, -1, 4)), dict(n=(4, 4, 0)), dict(cap=-1), dict(cap=65536),
               dict(n=(65537, 1, 1)), dict(n=(1, 65537, 1)), dict(n=(1, 1, 65537)), dict(n=(65536, 364, 1)), dict(n=(46342, 46342, 1)), dict(n=(2048, 2048, 512))):
        assert dist(**kw) == binding.ERR_ARG, kw
    assert (d2 == 77).all() and (stats == -5).all(), "a refused call writes nothing"
    assert dist(cap=65535) == 0 and dist(out=None) == 0 and dist(st=None) == 0 and stats.tolist() == [0, 64, -1]
    long_line = np.zeros(65536, np.int8)   # the longest line there is
    long_line[0] = 100
    d, s = binding.occ_distance_host(long_line)
    assert d[-1] == 65535 ** 2 == s[2] and np.array_equal(d, np.arange(65536, dtype=np.uint64) ** 2)
    # the cost table
    good = dict(inscribed_radius=0.3, inflation_radius=1.0, cost_scaling=3.0)
    table = np.full(26, 9, np.uint8)

    def tab(s=0.2, cap=26, t=table, **kw):
        return L.alego_occ_cost_table_host(s, C.byref(binding.occ_inflation(**dict(good, **kw))), None if t is None else t.ctypes.data, cap)

    for kw in (dict(s=0.0), dict(s=-0.2), dict(s=np.nan), dict(s=np.inf), dict(inscribed_radius=-0.1), dict(inscribed_radius=np.nan), dict(inflation_radius=np.inf),
               dict(inflation_radius=-1.0), dict(cost_scaling=-1.0), dict(cost_scaling=np.nan), dict(cost_scaling=np.inf), dict(inflation_radius=0.2),
               dict(s=0.25, inflation_radius=1024.0), dict(cap=-1), dict(t=None)):
        assert tab(**kw) == binding.ERR_ARG, kw
    assert L.alego_occ_cost_table_host(0.2, None, table.ctypes.data, 26) == binding.ERR_ARG
    assert tab(cap=25) == binding.ERR_CAPACITY and tab(cap=0, t=None) == binding.ERR_CAPACITY
    assert (table == 9).all(), "a refused call writes nothing"
    assert tab() == 26 and table[0] == 254
    assert tab(s=0.25, inflation_radius=1023.75, cap=4095 * 4095 + 1, t=np.zeros(4095 * 4095 + 1, np.uint8)) == 4095 * 4095 + 1   # r = 4095: the largest
    assert tab(inflation_radius=0.0, inscribed_radius=0.0, cap=1) == 1                                                           # r = 0: the source's entry alone
    # the cost rule
    out = np.full(64, 9, np.uint8)
    d2[:] = 1

    def cm(c=cls, d=d2, cells=64, t=table, n_table=26, o=out):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.alego_occ_costmap_host(ptr(c), ptr(d), cells, 0, ptr(t), n_table, 0, ptr(o))

    for kw in (dict(c=None), dict(d=None), dict(o=None), dict(t=None), dict(cells=-1), dict(n_table=0)):
        assert cm(**kw) == binding.ERR_ARG, kw
    assert (out == 9).all()
    assert cm() == 0 and (out == table[1]).all() and cm(c=None, d=None, o=None, cells=0) == 0


@pytest.mark.parametrize("case", range(len(TABLES)))
def test_cost_table_equals_numpy(case):
    s, inscribed, radius, scaling = TABLES[case]
    got = binding.occ_cost_table_host(s, binding.occ_inflation(inscribed, radius, scaling))
    want = ref.cost_table(s, inscribed, radius, scaling)
    r = int(np.ceil(radius / s))
    assert got.shape == want.shape == (r * r + 1,)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"table differs at d2 {bad[:5].tolist()}: got {got[bad[:5]].tolist()} want {want[bad[:5]].tolist()}"
    assert got[0] == 254 and (got[1:] <= 253).all() and (np.diff(got[1:].astype(int)) <= 0).all()
    assert (got[1:] == 253).sum() == int((np.sqrt(np.arange(1, r * r + 1)) * s <= inscribed).sum())


def test_cost_rule_cell_by_cell():
    infl = binding.occ_inflation(0.35, 2.0, 3.0)
    table = binding.occ_cost_table_host(0.2, infl)
    assert table.size == 101 and table[1] == 253 and table[3] == 253 and 0 < table[4] < 253   # sqrt(3) 0.2 = 0.346 <= 0.35 < 0.4
    # every class at: a source's own d2, the last inscribed d2, the first beyond it, the table's last entry, beyond the table, FAR
    d2 = np.array([0, 3, 4, 100, 101, 5000, ref.FAR], np.uint32)
    for uio in (False, True):
        for inflate in (False, True):
            for c in (100, 0, -1):
                cls = np.full(d2.shape, c, np.int8)
                got = binding.occ_costmap_host(cls, d2, table, uio, inflate)
                assert np.array_equal(got, ref.cost(cls, d2, table, uio, inflate)), (uio, inflate, c)
                t = [254, 253, int(table[4]), int(table[100]), 0, 0, 0]
                if c == 100 or (uio and c == -1):
                    assert got.tolist() == [254] * 7
                elif c == 0:
                    assert got.tolist() == t
                elif inflate:   # an unknown cell keeps every cost from 1 upwards
                    assert got.tolist() == [v if v >= 1 else 255 for v in t]
                else:           # ... or only the inscribed band: 253 stays, 252 and below are NO_INFORMATION
                    assert got.tolist() == [254, 253, 255, 255, 255, 255, 255]
    assert table[100] >= 1, "the table's last entry is still a cost at these parameters"
    # a whole grid: twin's d2 at the cap the device path uses, every combination of the flags
    rng = np.random.default_rng(9)
    cls = _random(rng, (3, 17, 23), 0.01)
    for uio in (False, True):
        d2, _ = binding.occ_distance_host(cls, uio, 10)
        for inflate in (False, True):
            got = binding.occ_costmap_host(cls, d2, table, uio, inflate)
            assert np.array_equal(got, ref.cost(cls, ref.distance(cls, uio, 10)[0], table, uio, inflate)), (uio, inflate)
            if not uio and not inflate:
                assert set(np.unique(got[cls == -1]).tolist()) == {253, 255}
