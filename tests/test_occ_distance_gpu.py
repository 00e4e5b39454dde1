"""The clearance field and the inflated cost map of the occupancy grid (alego_occ_distance, alego_occ_costmap) on the device.

Class patterns are set with alego_occ_set (a cell of class 100 has one hit, a free one one pass, an unknown one neither).  In every case the device's
d2 and statistics are compared for EXACT equality, over all cells, with the host twin alego_occ_distance_host fed by alego_occ_classify of the same
handle (the twin itself stands against brute force in tests/test_edt_math.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
INFLATIONS = ((0.2, 0.35, 2.0, 3.0), (0.4, 0.5, 3.0, 1.0))   # (s, inscribed, radius, scaling): two of the cost table's parameter sets


def _err(h):
    return binding.lib().alego_last_error(h._h).decode()


def _handle(p, n, cell=0.2, n_slots=1):
    """a mapping handle with the archive on and a grid of n = (n0, n1, n2) cells"""
    h = binding.Handle(p, n_slots=n_slots)
    h.map_enable(8, 4096)
    opts = binding.occ_opts((-1.0, 2.0, 0.5), cell, n)
    h.occ_enable(opts)
    return h


def _set(h, cls):
    """counts that classify to cls (n2, n1, n0) under the default rule"""
    h.occ_set((cls == 100).astype(np.uint32), (cls == 0).astype(np.uint32))


def _check(h, tag, collapse_z=False, unknown_is_obstacle=False, max_cells=0):
    """device against twin, d2 and statistics; returns them"""
    cls = h.occ_classify(collapse_z=collapse_z)
    want, ws = binding.occ_distance_host(cls, unknown_is_obstacle, max_cells)
    got, gs = h.occ_distance(None, collapse_z, unknown_is_obstacle, max_cells)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{tag}: d2 differs at {bad[:5].tolist()} of {bad.shape[0]}: got {got[got != want][:5].tolist()} want {want[got != want][:5].tolist()}"
    assert gs.tolist() == ws.tolist(), f"{tag}: stats {gs.tolist()} want {ws.tolist()}"
    return got, gs


def _patterns(shape, seed):
    """(name, classes (n2, n1, n0)): none, all, one corner, equidistant pairs, a checkerboard, a source only in the last cell of the last line, random"""
    rng = np.random.default_rng(seed)
    base = rng.choice(np.array([0, -1], np.int8), size=shape)
    out = [("none", base.copy()), ("all", np.full(shape, 100, np.int8))]
    c = base.copy(); c[0, 0, 0] = 100
    out.append(("one corner", c))
    c = base.copy()
    for axis in range(3):   # two sources at the ends of the middle line of each axis: the cells between see both
        i = [m // 2 for m in shape]
        i[axis] = 0; c[tuple(i)] = 100
        i[axis] = shape[axis] - 1; c[tuple(i)] = 100
    out.append(("equidistant pairs", c))
    z, y, x = np.indices(shape)
    out.append(("checkerboard", np.where((x + y + z) % 2 == 0, 100, base).astype(np.int8)))
    c = base.copy(); c[-1, -1, -1] = 100
    out.append(("last cell", c))
    for density in (0.01, 0.3):
        c = base.copy(); c[rng.random(shape) < density] = 100
        out.append((f"random {density}", c))
    return out


# pass X's wavefront and carry edges (n0), the line lengths of passes Y and Z (n1, n2), their lane counts (lines = n0 n2 of pass Y: 1, 63, 64, 65)
GRIDS = [(1, 3, 2), (63, 3, 2), (64, 3, 2), (65, 3, 2), (129, 3, 2), (257, 3, 2),
         (5, 1, 3), (5, 2, 3), (5, 3, 3), (5, 64, 3), (5, 65, 3), (5, 257, 3),
         (5, 3, 1), (5, 3, 2), (5, 3, 64), (5, 3, 65), (5, 3, 257),
         (1, 7, 1), (63, 7, 1), (64, 7, 1), (65, 7, 1), (9, 5, 7), (13, 6, 5), (1, 1, 1), (37, 29, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "x".join(str(v) for v in n))
def test_patterns_equal_the_twin(params_a, n):
    h = _handle(params_a, n)
    seen_far = seen_finite = False
    for name, cls in _patterns(n[::-1], seed=sum(n)):
        _set(h, cls)
        assert np.array_equal(h.occ_classify(), cls), name
        d2, stats = _check(h, f"{n} {name}")
        seen_far |= bool(stats[binding.EDT_FAR_CELLS]); seen_finite |= stats[binding.EDT_MAX_D2] >= 0
        if name == "all":
            assert not d2.any() and stats.tolist() == [cls.size, 0, 0]
        if name == "none":
            assert (d2 == binding.OCC_FAR).all() and stats.tolist() == [0, cls.size, -1]
        if name == "last cell":
            assert d2[0, 0, 0] == sum((m - 1) ** 2 for m in n) == stats[binding.EDT_MAX_D2]
    assert seen_far and seen_finite
    h.close()


@pytest.fixture(scope="module")
def grid_37(params_a):
    h = _handle(params_a, (37, 29, 5))
    yield h
    h.close()


@pytest.mark.gpu
def test_options(grid_37):
    h = grid_37
    rng = np.random.default_rng(12)
    cls = rng.choice(np.array([0, -1], np.int8), size=(5, 29, 37))
    cls[rng.random(cls.shape) < 0.004] = 100
    _set(h, cls)
    free, stats = _check(h, "no options")
    for cap in (1, 3):
        d2, s = _check(h, f"cap {cap}", max_cells=cap)
        assert ((d2 == binding.OCC_FAR) == (free > cap * cap)).all() and s[binding.EDT_MAX_D2] == cap * cap
    unk, s = _check(h, "unknown_is_obstacle", unknown_is_obstacle=True)
    assert s[binding.EDT_SOURCES] == int((cls != 0).sum()) and (unk < free).any()
    _check(h, "unknown_is_obstacle, cap 3", unknown_is_obstacle=True, max_cells=3)
    # collapsed against flat: the collapsed call equals the twin of the collapsed classes, and differs from every layer's own field
    col, cs = _check(h, "collapsed", collapse_z=True)
    assert col.shape == (29, 37) and cs[binding.EDT_SOURCES] == int((cls == 100).any(axis=0).sum()) and (col <= free.min(axis=0)).all()
    _check(h, "collapsed, cap 3, unknown", collapse_z=True, unknown_is_obstacle=True, max_cells=3)
    again, _ = _check(h, "flat after collapsed")
    assert np.array_equal(again, free)
    # count-only: d2 = NULL gives the statistics alone
    none, only = h.occ_distance(want_d2=False)
    assert none is None and only.tolist() == stats.tolist()
    # a rule other than the default reaches the classification
    h.occ_set((cls == 100).astype(np.uint32) * 3, (cls != -1).astype(np.uint32) * 4)
    got, gs = h.occ_distance((1, 1, 1))
    want, ws = binding.occ_distance_host(h.occ_classify((1, 1, 1)))
    assert np.array_equal(got, want) and gs.tolist() == ws.tolist() and gs[binding.EDT_SOURCES] == 0
    got, gs = h.occ_distance((1, 2, 1))
    assert np.array_equal(got, free) and gs.tolist() == stats.tolist()


@pytest.mark.gpu
def test_state_carried_between_calls(params_a, grid_37):
    h = grid_37
    rng = np.random.default_rng(3)
    a = np.where(rng.random((5, 29, 37)) < 0.3, 100, 0).astype(np.int8)
    b = np.full((5, 29, 37), -1, np.int8); b[4, 28, 36] = 100
    _set(h, a)
    first, s1 = _check(h, "dense")
    again, s2 = _check(h, "the same call twice")
    assert np.array_equal(first, again) and s1.tolist() == s2.tolist()
    _set(h, b)   # far fewer sources: nothing of the dense field may stay
    sparse, s3 = _check(h, "sparse after dense")
    assert s3.tolist() == [1, 0, 36 * 36 + 28 * 28 + 4 * 4] and sparse[0, 0, 0] == s3[2]
    _check(h, "collapsed after flat", collapse_z=True)
    _set(h, a)
    back, _ = _check(h, "dense again")
    assert np.array_equal(back, first)
    # a larger grid's call after a smaller one, on another handle
    small, large = _handle(params_a, (7, 5, 3)), _handle(params_a, (70, 45, 9))
    for hh, shape in ((small, (3, 5, 7)), (large, (9, 45, 70)), (small, (3, 5, 7))):
        c = np.where(rng.random(shape) < 0.02, 100, -1).astype(np.int8)
        c[0, 0, 0] = 100
        _set(hh, c)
        _check(hh, f"{shape}")
        _check(hh, f"{shape} collapsed", collapse_z=True)
    small.close(); large.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(INFLATIONS)))
def test_costmap_equals_the_twin(params_a, case):
    s, inscribed, radius, scaling = INFLATIONS[case]
    h = _handle(params_a, (37, 29, 5), cell=s)
    rng = np.random.default_rng(40 + case)
    cls = rng.choice(np.array([0, -1], np.int8), size=(5, 29, 37))
    cls[..., :10][rng.random((5, 29, 10)) < 0.01] = 100   # sources at low x only: the far side lies beyond the inflation radius
    _set(h, cls)
    seen = set()
    for collapse in (False, True):
        c = h.occ_classify(collapse_z=collapse)
        for uio in (False, True):
            for inflate in (False, True):
                infl = binding.occ_inflation(inscribed, radius, scaling, inflate)
                table = binding.occ_cost_table_host(s, infl)
                r = int(np.ceil(radius / s))
                assert table.size == r * r + 1
                d2, _ = binding.occ_distance_host(c, uio, r)
                want = binding.occ_costmap_host(c, d2, table, uio, inflate)
                got = h.occ_costmap(infl, None, collapse, uio)
                bad = np.argwhere(got != want)
                assert bad.shape[0] == 0, f"{(collapse, uio, inflate)}: costs differ at {bad[:5].tolist()}: got {got[got != want][:5].tolist()} want {want[got != want][:5].tolist()}"
                seen |= set(np.unique(got).tolist())
    assert {254, 253, 255, 0} <= seen and len(seen) > 6
    h.close()


@pytest.mark.gpu
def test_every_refusal(params_a):
    L = binding.lib()
    d2, stats, out = np.zeros(37 * 29 * 5, np.uint32), np.zeros(3, np.int64), np.zeros(37 * 29 * 5, np.uint8)
    infl = binding.occ_inflation(0.3, 1.0, 3.0)

    def calls(h):
        return (L.alego_occ_set(h._h, d2.ctypes.data, None), L.alego_occ_distance(h._h, None, None, d2.ctypes.data, stats.ctypes.data),
                L.alego_occ_costmap(h._h, None, 0, 0, C.byref(infl), out.ctypes.data))

    h = binding.Handle(params_a)
    assert calls(h) == (binding.ERR_ARG,) * 3 and "archive is off" in _err(h)      # archive off
    h.map_enable(8, 4096)
    assert calls(h) == (binding.ERR_ARG,) * 3 and "alego_occ_enable" in _err(h)    # before enable
    assert L.alego_occ_distance(None, None, None, d2.ctypes.data, None) == binding.ERR_ARG and L.alego_occ_set(None, None, None) == binding.ERR_ARG
    h.occ_enable(binding.occ_opts((0, 0, 0), (0.2, 0.2, 0.2), (37, 29, 5)))
    assert calls(h) == (0,) * 3
    assert L.alego_occ_set(h._h, None, None) == 0 and L.alego_occ_distance(h._h, None, None, None, None) == 0

    def dist(rule=None, **kw):
        o = binding.OccDistOpts(kw.get("collapse_z", 0), kw.get("unknown_is_obstacle", 0), kw.get("max_cells", 0), 0)
        return L.alego_occ_distance(h._h, None if rule is None else C.byref(binding.OccRule(*rule, 0)), C.byref(o), d2.ctypes.data, stats.ctypes.data)

    d2[:] = 77; stats[:] = -5
    for kw in (dict(max_cells=-1), dict(max_cells=65536), dict(rule=(-1, 2, 1)), dict(rule=(1, -2, 1)), dict(rule=(1, 2, -1))):
        assert dist(**kw) == binding.ERR_ARG and _err(h), kw
    assert (d2 == 77).all() and (stats == -5).all(), "a refused call writes nothing"
    assert dist(max_cells=65535) == 0

    def cost(collapse_z=0, rule=None, i=infl, o=out, **kw):
        i = binding.occ_inflation(**kw) if kw else i
        return L.alego_occ_costmap(h._h, None if rule is None else C.byref(binding.OccRule(*rule, 0)), collapse_z, 0, None if i is None else C.byref(i),
                                   None if o is None else o.ctypes.data)

    out[:] = 9
    for kw in (dict(i=None), dict(o=None), dict(rule=(-1, 2, 1)), dict(inscribed_radius=-0.1, inflation_radius=1.0), dict(inscribed_radius=np.nan, inflation_radius=1.0),
               dict(inscribed_radius=0.3, inflation_radius=np.inf), dict(inscribed_radius=0.3, inflation_radius=1.0, cost_scaling=-1.0),
               dict(inscribed_radius=0.3, inflation_radius=1.0, cost_scaling=np.nan), dict(inscribed_radius=0.3, inflation_radius=0.2),
               dict(inscribed_radius=0.3, inflation_radius=819.3)):
        assert cost(**kw) == binding.ERR_ARG, kw
    assert (out == 9).all()
    h.close()
    # unequal cell sizes on axes with more than one cell; one thick layer and a collapsed grid need only cell[0] == cell[1]
    for cell, n, flat_ok, collapsed_ok in (((0.2, 0.2, 0.5), (6, 5, 4), False, True), ((0.2, 0.25, 0.2), (6, 5, 4), False, False), ((0.2, 0.2, 3.0), (6, 5, 1), True, True),
                                           ((0.2, 0.3, 0.2), (6, 1, 4), True, True), ((0.7, 0.3, 0.5), (1, 1, 4), True, True), ((0.2, 0.3, 0.2), (6, 5, 1), False, False)):
        g = binding.Handle(params_a)
        g.map_enable(8, 4096)
        g.occ_enable(binding.occ_opts((0, 0, 0), cell, n))
        for collapse, ok in ((0, flat_ok), (1, collapsed_ok)):
            o = binding.OccDistOpts(collapse, 0, 0, 0)
            rc = L.alego_occ_distance(g._h, None, C.byref(o), d2.ctypes.data, stats.ctypes.data)
            assert rc == (0 if ok else binding.ERR_ARG), (cell, n, collapse)
            assert ok or "edge length" in _err(g)
            assert L.alego_occ_costmap(g._h, None, collapse, 0, C.byref(infl), out.ctypes.data) == (0 if ok else binding.ERR_ARG), (cell, n, collapse)
        g.close()
    # a 65 537-cell line
    g = binding.Handle(params_a)
    g.map_enable(8, 4096)
    g.occ_enable(binding.occ_opts((0, 0, 0), 0.2, (65537, 1, 1)))
    big = np.zeros(65537, np.uint32)
    assert L.alego_occ_distance(g._h, None, None, big.ctypes.data, None) == binding.ERR_ARG and "2^32 - 2" in _err(g)
    g.close()


@pytest.mark.gpu
def test_longest_line(params_a):
    """65 536 cells along x: 1 024 blocks of pass X, the largest g^2"""
    h = _handle(params_a, (65536, 1, 1))
    cls = np.zeros((1, 1, 65536), np.int8)
    cls[0, 0, 0] = 100
    _set(h, cls)
    d2, stats = _check(h, "source at 0")
    assert d2[0, 0, -1] == 65535 ** 2 == stats[binding.EDT_MAX_D2]
    cls[0, 0, 0] = 0; cls[0, 0, 40000] = 100
    _set(h, cls)
    _check(h, "source at 40000")
    h.close()


@pytest.mark.gpu
def test_localising_handle_is_refused(params_a):
    rng = np.random.default_rng(4)
    cloud = lambda n: np.concatenate([rng.uniform(-9, 9, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
    h = binding.Handle(params_a)
    h.loc_enable([(np.zeros(6, np.float32), cloud(20), cloud(60), cloud(20))])
    L = binding.lib()
    d2, out = np.zeros(8, np.uint32), np.zeros(8, np.uint8)
    infl = binding.occ_inflation(0.3, 1.0, 3.0)
    assert L.alego_occ_distance(h._h, None, None, d2.ctypes.data, None) == binding.ERR_ARG and "localising" in _err(h)
    assert L.alego_occ_costmap(h._h, None, 0, 0, C.byref(infl), out.ctypes.data) == binding.ERR_ARG and "localising" in _err(h)
    assert L.alego_occ_set(h._h, d2.ctypes.data, None) == binding.ERR_ARG and "localising" in _err(h)
    h.close()


@pytest.mark.gpu
def test_stream_is_untouched():
    """60 scans of the synthetic stream on two 2-slot handles with the grid enabled; one integrates and calls the new functions every 20 scans"""
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(60)]
    opts = binding.occ_opts(origin=(-40.0, -40.0, -3.0), cell=(0.5, 0.5, 0.5), n=(160, 160, 12), min_range=1.0, max_range=35.0)
    infl = binding.occ_inflation(0.35, 2.0, 3.0)

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
        results = []
        for first in (0, 20, 40):
            h.batch_run(first, 20, stages=7 | binding.REPLAY_BAG, sync=True)
            if with_calls:
                h.occ_clear()
                h.occ_integrate(slot=0); h.occ_integrate(slot=1)
                results.append((h.occ_distance(), h.occ_distance(collapse_z=True, max_cells=10), h.occ_costmap(infl, collapse_z=True)))
        names = list(h.profile_report())
        h.profile_enable(False)
        return h, names, results

    (a, names_a, _), (b, names_b, results) = run(False), run(True)
    assert not [n for n in names_a if n.startswith("edt_")], "none of the new kernels runs on a handle that never calls them"
    assert {"edt_pass_x", "edt_pass_y", "edt_pass_z", "edt_finish", "edt_cost_k"} <= set(names_b)
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
    # the grid's counts: a integrates once at the end what b integrated after its last clear; the new calls changed nothing
    a.occ_integrate(slot=0); a.occ_integrate(slot=1)
    for ga, gb, name in zip(a.occ_get(), b.occ_get(), ("hits", "passes")):
        assert np.array_equal(ga, gb), name
    # ... and the last results equal the twins of that grid
    (d2, st), (col, cst), cost = results[-1]
    want, ws = binding.occ_distance_host(b.occ_classify())
    assert np.array_equal(d2, want) and st.tolist() == ws.tolist() and st[binding.EDT_SOURCES] > 100
    cc = b.occ_classify(collapse_z=True)
    want, ws = binding.occ_distance_host(cc, False, 10)
    assert np.array_equal(col, want) and cst.tolist() == ws.tolist()
    assert np.array_equal(cost, binding.occ_costmap_host(cc, want, binding.occ_cost_table_host(0.5, infl)))
    a.close(); b.close()


@pytest.mark.gpu
def test_replay_writes_the_costmap(tmp_path):
    exe = os.path.join(ROOT, "examples", "replay")
    r = subprocess.run([exe, "60", "--occupancy", "0.5", str(tmp_path), "--inflate", "0.35", "2.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("occupancy: ")][0].split()
    f = dict(origin=[float(v) for v in line[2:5]], cell=[float(v) for v in line[6:9]], n=[int(v) for v in line[10:13]], max_range=float(line[14]))
    cm = [ln for ln in r.stdout.splitlines() if ln.startswith("costmap: ")][0].split()
    assert cm[1::2] == ["r", "sources", "far", "max_d2", "lethal", "inscribed", "unknown"]
    printed = dict(zip(cm[1::2], (int(v) for v in cm[2::2])))
    p = synth.default_params(16, 1800)
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    for k in range(60):
        h.scan_process(synth.scan(p, k), stages=7, stamp=0.1 * k)
    h.occ_enable(binding.occ_opts(f["origin"], f["cell"], f["n"], 0.0, f["max_range"]))
    h.occ_integrate()
    infl = binding.occ_inflation(0.35, 2.0, 10.0)   # SCALING defaults to 10
    want = h.occ_costmap(infl, collapse_z=True)
    _, stats = h.occ_distance(collapse_z=True, max_cells=4, want_d2=False)
    assert printed == dict(r=4, sources=int(stats[0]), far=int(stats[1]), max_d2=int(stats[2]), lethal=int((want == 254).sum()), inscribed=int((want == 253).sum()),
                           unknown=int((want == 255).sum()))
    # (no cell is inscribed: the nearest neighbour of a source lies 0.5 m away, beyond the 0.35 m)
    assert printed["lethal"] == printed["sources"] > 0 and printed["inscribed"] == 0 and printed["unknown"] > 0 and ((want > 0) & (want < 253)).any()
    raw = open(tmp_path / "costmap.pgm", "rb").read()
    head = f"P5\n{f['n'][0]} {f['n'][1]}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + f["n"][0] * f["n"][1]
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(f["n"][1], f["n"][0])
    assert np.array_equal(img[::-1], want)   # rows as occupancy.pgm orders them: the top row is the largest y
    assert os.path.exists(tmp_path / "occupancy.pgm")
    # without --occupancy it is a usage error
    r = subprocess.run([exe, "5", "--inflate", "0.35", "2.0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--occupancy" in r.stderr
    h.close()
