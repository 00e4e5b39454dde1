"""A slot's key-frame archive thinned in place on the device (alego_map_thin, kernels_thin.hip / thin_math.h).

The selection rule and the graph of the kept frames have host twins (alego_map_thin_select, alego_map_thin_edges) that are checked without a
GPU against restatements in Python: the selection on integer-lattice positions, where the f32 squared distance is exact, and the edges in plain
Python floats (IEEE f64, no contraction) in the stated association order, so both must agree EXACTLY.

Every device comparison is made against a replica built in a fresh slot of the same handle by public calls only (host_thin below):
alego_lm_reset_window, alego_lm_add_keyframe of every kept frame as read back before the thin, alego_map_set_stamps, alego_graph_set_edges
with alego_map_thin_edges' chain, alego_graph_add_edge(.., NULL) for the remapped loops - byte for byte over every public getter.  loop_closed_
and the estimate count are compared with the rule (unchanged / 0), lm_state with the slot's own state before the thin (untouched).
"""
import os
import re
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from test_loop_appearance import MAX_RANGE, Z_OFFSET
from test_loop_search import _params, _scan
from test_map_align import rigid
from test_map_merge import EMPTY, ITEM, K, ODOM_VAR, SEAM, add, archived_poses, compose_py, graph_on, rand_clouds, same, snap
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["alego_map_thin", "alego_map_thin_select", "alego_map_thin_edges", "alego_debug_thin_select"]
LDS_KEPT = 2048             # TH_LDS_KEPT of csrc/thin_math.h: kept positions th_select holds in LDS


# ---- the rule restated --------------------------------------------------------------------------------------------------------------
def select_py(kp, protect, min_dist):
    """the selection rule in numpy f32, one frame at a time: ((dx dx) + dy dy) + dz dz < (float)(min_dist * min_dist) against every kept j < i"""
    kp = np.asarray(kp, F32).reshape(-1, 6)
    n = kp.shape[0]
    keep = np.zeros(n, np.uint8)
    r2 = F32(np.float64(min_dist) * np.float64(min_dist))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            drop = False
            if not protect[i] and min_dist > 0:
                j = np.nonzero(keep[:i])[0]
                d = kp[i, :3][None, :] - kp[j, :3]
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                assert d2.dtype == F32
                drop = bool((d2 < r2).any())
            keep[i] = 0 if drop else 1
    return keep


def _kp(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.c_[xyz, np.zeros((len(xyz), 3))].astype(F32)


def lattice_cases():
    """(name, key poses (n, 6) on the integer lattice, protect (n,), min_dist, expected keep or None)"""
    nan = np.nan
    up = float(np.sqrt(np.float64(np.nextafter(F32(25), F32(26)))))   # (float)(up * up) is the f32 after 25
    assert F32(up * up) == np.nextafter(F32(25), F32(26)) and F32(5.0 * 5.0) == F32(25)
    none = lambda n: np.zeros(n, np.uint8)
    cases = [
        ("a pair at exactly r^2 stays", _kp([[0, 0, 0], [3, 4, 0]]), none(2), 5.0, [1, 1]),
        ("a pair one f32 below r^2 goes", _kp([[0, 0, 0], [3, 4, 0]]), none(2), up, [1, 0]),
        ("exactly r^2 in three axes", _kp([[1, 2, 3], [3, 5, 9]]), none(2), 7.0, [1, 1]),
        ("greedy: B dropped by A suppresses nobody, C stays", _kp([[0, 0, 0], [2, 0, 0], [4, 0, 0]]), none(3), 3.0, [1, 0, 1]),
        ("one place: frame 0 and the protected frames", _kp([[1, 1, 1]] * 8), np.array([0, 0, 1, 0, 0, 1, 0, 0], np.uint8), 0.5, [1, 0, 1, 0, 0, 1, 0, 0]),
        ("a protected frame in the middle suppresses later frames", _kp([[0, 0, 0], [10, 0, 0], [10, 1, 0], [0, 1, 0], [10, 0, 1]]), np.array([0, 1, 0, 0, 0], np.uint8), 2.0, [1, 1, 0, 0, 0]),
        ("a NaN position is kept and suppresses nothing", _kp([[0, 0, 0], [nan, 0, 0], [nan, 0, 0], [0, 0, 1], [0, nan, 5]]), none(5), 2.0, [1, 1, 1, 0, 1]),
        ("an infinite position", _kp([[0, 0, 0], [np.inf, 0, 0], [np.inf, 0, 0]]), none(3), 2.0, [1, 1, 1]),
        ("min_dist 0", _kp([[0, 0, 0]] * 4), none(4), 0.0, [1, 1, 1, 1]),
        ("min_dist negative", _kp([[0, 0, 0]] * 4), none(4), -3.0, [1, 1, 1, 1]),
        ("n = 1", _kp([[7, 8, 9]]), none(1), 100.0, [1]),
        ("n = 1, protected", _kp([[7, 8, 9]]), np.ones(1, np.uint8), 100.0, [1]),
    ]
    return cases


def random_lattice(n, seed):
    """n frames on a small integer lattice (many coincide or lie at lattice distances 1, sqrt 2, sqrt 3, 2), one in ten protected"""
    rng = np.random.default_rng(seed)
    side = max(2, int(round((n / 3.0) ** (1 / 3.0))) + 1)
    kp = _kp(rng.integers(0, side, (n, 3)) * 2)
    protect = (rng.random(n) < 0.1).astype(np.uint8)
    return kp, protect, (2.0, 2.5, 3.0)[seed % 3]     # 2.0: a neighbour at exactly r^2 stays


N_CASES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def edges_py(chain, loops, keep):
    """the graph of the kept frames in Python floats: edge m = ((E_(a+1) E_(a+2)) ...) E_b, variances summed in that order"""
    kept = [i for i in range(len(keep)) if keep[i]]
    new_id = {o: m for m, o in enumerate(kept)}
    frm, to, btw, var = [-1], [0], [np.asarray(chain["between"][0], np.float64)], [[float(v) for v in chain["variance"][0]]]
    for m in range(1, len(kept)):
        a, b = kept[m - 1], kept[m]
        B, V = np.asarray(chain["between"][a + 1], np.float64), [float(v) for v in chain["variance"][a + 1]]
        for f in range(a + 2, b + 1):
            B = compose_py(B, chain["between"][f])
            V = [V[k] + float(chain["variance"][f][k]) for k in range(6)]
        frm.append(m - 1); to.append(m); btw.append(B); var.append(V)
    oc = dict(frm=np.array(frm, np.int64), to=np.array(to, np.int64), between=np.array(btw).reshape(-1, 3, 4), variance=np.array(var).reshape(-1, 6))
    nl = len(loops["frm"])
    ol = dict(frm=np.array([new_id[int(a)] for a in loops["frm"]], np.int64), to=np.array([new_id[int(b)] for b in loops["to"]], np.int64),
              between=np.asarray(loops["between"], np.float64).reshape(nl, 3, 4), variance=np.asarray(loops["variance"], np.float64).reshape(nl, 6))
    return oc, ol


def _edges(rng, frm, to):
    n = len(frm)
    return dict(frm=np.asarray(frm, np.int64), to=np.asarray(to, np.int64),
                between=np.array([rigid(rng.uniform(-0.3, 0.3, 3), rng.uniform(-3, 3, 3))[:3] for _ in range(n)], np.float64).reshape(n, 3, 4), variance=rng.uniform(1e-8, 1e-2, (n, 6)))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_thin_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s
    for t in ("alego_map_thin_opts", "alego_map_thin_result", "FIRST-ORDER rule", "Out of scope"):
        assert t in hdr, t
    assert "removing duplicate frames of the overlap" not in hdr, "the merge's out-of-scope line is reworded"
    src = open(os.path.join(ROOT, "a-lego-loam_amd", "csrc", "thin_math.h")).read()
    assert int(re.search(r"#define TH_LDS_KEPT (\d+)", src).group(1)) == LDS_KEPT


@pytest.mark.parametrize("case", lattice_cases(), ids=lambda c: c[0])
def test_select_twin_equals_the_restatement_on_the_lattice(case):
    name, kp, protect, min_dist, want = case
    got = binding.map_thin_select(kp, protect, min_dist)
    assert got.tolist() == select_py(kp, protect, min_dist).tolist() == want, name


@pytest.mark.parametrize("n", N_CASES)
def test_select_twin_equals_the_restatement_on_random_lattices(n):
    dropped = 0
    for seed in range(3):
        kp, protect, md = random_lattice(n, 100 * n + seed)
        got, want = binding.map_thin_select(kp, protect, md), select_py(kp, protect, md)
        assert got.tolist() == want.tolist(), (n, seed)
        assert got[0] == 1 and (got[protect != 0] == 1).all()
        dropped += int((got == 0).sum())
    assert n < 63 or dropped > 0
    L = binding.lib()
    keep = np.zeros(4, np.uint8)
    assert L.alego_map_thin_select(None, None, 2, 1.0, keep.ctypes.data) == binding.ERR_ARG
    assert L.alego_map_thin_select(_kp([[0, 0, 0]]).ctypes.data, None, 1, float("nan"), keep.ctypes.data) == binding.ERR_ARG
    assert L.alego_map_thin_select(_kp([[0, 0, 0]]).ctypes.data, None, -1, 1.0, keep.ctypes.data) == binding.ERR_ARG
    assert L.alego_map_thin_select(None, None, 0, 1.0, None) == 0
    two = _kp([[0, 0, 0], [0, 0, 0]])
    assert L.alego_map_thin_select(two.ctypes.data, None, 2, 1.0, keep.ctypes.data) == 1 and keep[:2].tolist() == [1, 0], "no protect mask: no frame protected"


def test_edges_twin_equals_python_floats():
    """alego_map_thin_edges against the restatement in Python floats: ids, order, measurements and variances exactly equal"""
    rng = np.random.default_rng(7)
    for n, nl in ((1, 0), (2, 0), (5, 1), (12, 3), (40, 6)):
        ch = _edges(rng, np.arange(n) - 1, np.arange(n))
        keep = (rng.random(n) < 0.5).astype(np.uint8)
        keep[0] = 1
        ends = rng.integers(0, n, (nl, 2))
        ends[:, 1] = np.where(ends[:, 1] == ends[:, 0], (ends[:, 0] + 1) % n, ends[:, 1])
        keep[ends.reshape(-1)] = 1
        lp = _edges(rng, ends[:, 0], ends[:, 1])
        for kp_ in (keep, np.ones(n, np.uint8), np.r_[1, np.zeros(n - 1)].astype(np.uint8) if nl == 0 else keep):
            oc, ol = binding.map_thin_edges(ch, lp, kp_)
            wc, wl = edges_py(ch, lp, kp_)
            for got, want, what in ((oc, wc, "chain"), (ol, wl, "loops")):
                assert got["frm"].tolist() == want["frm"].tolist() and got["to"].tolist() == want["to"].tolist(), (n, what)
                assert_bit_equal(got["between"], want["between"], f"{what}: measurements (n = {n})")
                assert_bit_equal(got["variance"], want["variance"], f"{what}: variances (n = {n})")
            assert len(oc["frm"]) == int(kp_.sum())
        oc, _ = binding.map_thin_edges(ch, lp, np.ones(n, np.uint8))
        assert_bit_equal(oc["between"], ch["between"], "nothing dropped: every measurement stays what was measured")
        assert_bit_equal(oc["variance"], ch["variance"], "nothing dropped: variances")
    ch, lp = _edges(rng, np.arange(4) - 1, np.arange(4)), _edges(rng, [3], [1])
    for bad in ([0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 0]):   # frame 0 dropped; an endpoint of the loop edge dropped
        with pytest.raises(binding.AlegoError):
            binding.map_thin_edges(ch, lp, bad)
    with pytest.raises(binding.AlegoError):
        binding.map_thin_edges(ch, _edges(rng, [4], [1]), [1, 1, 1, 1])


def test_thin_math_stand_alone(tmp_path):
    """tests/thin_math/thin_math_check.cpp over csrc/thin_math.h, built with AddressSanitizer and UBSan as a program of its own"""
    exe = str(tmp_path / "thin_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "thin_math", "thin_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "thin_math ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


# ---- GPU: th_select alone -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=1)
    yield h
    h.close()


@pytest.mark.gpu
def test_select_kernel_equals_the_twin(dev):
    """alego_debug_thin_select equals alego_map_thin_select mask for mask: the lattice cases, random lattices of every n at which the wavefront's
    chunks change (one lane, one chunk, one more), and more kept frames than the LDS staging holds - with frames dropped by kept frames on both
    sides of that limit"""
    for name, kp, protect, md, want in lattice_cases():
        assert dev.debug_thin_select(kp, protect, md).tolist() == want, name
    for n in N_CASES:
        for seed in range(3):
            kp, protect, md = random_lattice(n, 100 * n + seed)
            assert dev.debug_thin_select(kp, protect, md).tolist() == binding.map_thin_select(kp, protect, md).tolist(), (n, seed)
    n = LDS_KEPT + 600
    xyz = np.c_[np.arange(n) * 4.0, np.zeros(n), np.zeros(n)]
    xyz[LDS_KEPT + 300:LDS_KEPT + 450] = xyz[LDS_KEPT + 100:LDS_KEPT + 250]     # dropped by kept frames that are read from the poses
    xyz[LDS_KEPT + 450:] = xyz[10:160] + [0, 1, 0]                              # dropped by kept frames that are in LDS
    xyz[LDS_KEPT + 599] = [-50, 0, 0]
    kp, protect = _kp(xyz), np.zeros(n, np.uint8)
    protect[LDS_KEPT + 320] = 1
    got, want = dev.debug_thin_select(kp, protect, 2.0), binding.map_thin_select(kp, protect, 2.0)
    assert got.tolist() == want.tolist()
    assert int(want.sum()) == n - 300 + 2 and want[LDS_KEPT + 320] == 1 and want[LDS_KEPT + 599] == 1 and int(want[:LDS_KEPT + 300].sum()) > LDS_KEPT
    assert dev.debug_thin_select(np.zeros((0, 6), F32), np.zeros(0, np.uint8), 1.0).tolist() == []
    with pytest.raises(binding.AlegoError):
        dev.debug_thin_select(kp[:2], protect[:2], float("inf"))


# ---- GPU: the replica ------------------------------------------------------------------------------------------------------------------
def protect_mask(h, s, k=K):
    n = h.map_status(s)[0]
    p = np.zeros(n, np.uint8)
    if n:
        p[0] = 1
        p[max(0, n - (k + 1)):] = 1
        if graph_on(h):
            lp = h.graph_get_edges(kind=1, slot=s)
            p[np.r_[lp["frm"], lp["to"]].astype(int)] = 1
    return p


def expected_keep(h, s, min_dist, k=K):
    return binding.map_thin_select(archived_poses(h, s), protect_mask(h, s, k), min_dist)


def host_thin(h, s, rep, keep):
    """the replica of slot s thinned by `keep`, built in the fresh slot rep by public calls only"""
    ids = [i for i in range(len(keep)) if keep[i]]
    frames = [h.map_get_keyframe(f, slot=s) for f in ids]
    stamps = h.map_get_stamps(slot=s)[ids]
    assert h.map_status(rep)[0] == 0 and h.lm_keyframe_count(slot=rep) == 0, "a fresh slot"
    h.lm_reset_window(slot=rep)
    for f in frames:
        h.lm_add_keyframe(f["pose"], f["corner"], f["surf"], f["outlier"], slot=rep)
    h.map_set_stamps(0, stamps, slot=rep)
    if graph_on(h):
        ch, lp = binding.map_thin_edges(h.graph_get_edges(kind=0, slot=s), h.graph_get_edges(kind=1, slot=s), keep)
        h.graph_set_edges(0, ch["frm"], ch["to"], ch["between"], ch["variance"], slot=rep)
        for i in range(len(lp["frm"])):
            h.graph_add_edge(int(lp["frm"][i]), int(lp["to"][i]), lp["between"][i], lp["variance"][i], slot=rep)


RULE = ("graph_status", "the graph's estimate", "lm_state")   # compared with the rule, not with the replica


def snap_vs_replica(h, s, k=K):
    return [(n, v) for n, v in snap(h, s, k) if n not in RULE]


def check_thinned(h, s, rep, before, tag, k=K):
    """slot s after the thin against its replica; `before`: snap(h, s) taken before the thin"""
    same(snap_vs_replica(h, s, k), snap_vs_replica(h, rep, k), f"{tag}: slot {s} against its replica {rep}")
    b = dict(before)
    assert_bit_equal(h.debug_get("lm_state", slot=s), b["lm_state"], f"{tag}: slot {s}: map -> odom and params_ are untouched")
    if graph_on(h):
        gs, gr = h.graph_status(s), h.graph_status(rep)
        assert tuple(gs[:2]) == tuple(gr[:2]) == (h.map_status(s)[0], int(b["graph_status"][1])), (tag, s, gs, gr)
        assert gs[2] == int(b["graph_status"][2]), f"{tag}: slot {s}: loop_closed_ stays as it was"
        assert gs[3] == 0, f"{tag}: slot {s}: the last estimate is discarded"


def line_poses(rng, n, dups=None, step=3.0):
    """key poses 3 m apart on a line with random small roll / pitch and any yaw; dups {i: j}: frame i at the position of frame j"""
    po = np.c_[np.arange(n) * step, np.zeros(n), np.zeros(n), rng.uniform(-0.05, 0.05, (n, 2)), rng.uniform(-3, 3, (n, 1))].astype(F32)
    for i, j in sorted((dups or {}).items()):
        po[i, :3] = po[j, :3]
    return po


def cloud(rng, n):
    return np.c_[rng.uniform(-40, 40, (n, 3)), rng.uniform(0, 16, (n, 1))].astype(F32)


def loop_edge(h, s, a, b, rng):
    h.graph_add_edge(int(a), int(b), rigid(rng.uniform(-0.1, 0.1, 3), rng.uniform(-2, 2, 3))[:3], rng.uniform(1e-4, 1e-2, 6), slot=s)


MIN_DIST = 1.0


@pytest.mark.gpu
def test_thin_equals_the_replica_for_every_shape():
    """N in {1, K, K + 1, K + 2, 2 K + 3, 40} and the point-count edges of the copy, in ONE call over both stream groups of a 128-slot handle.
    Every slot with a dropped frame against its replica; the slots with nothing to drop byte-unchanged; the slots not listed byte-unchanged."""
    import pose_graph_ref as R
    rng = np.random.default_rng(61)
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=128)
    try:
        assert h.stream_groups()[1] == 64
        h.map_enable(40, 1 << 14)
        h.graph_enable(8, ODOM_VAR)
        big = 3 * ITEM + 37
        frames90 = [cloud(rng, 90) for _ in range(12)]
        frames90[2] = cloud(rng, big)                                # a kept frame of three copy items + 37 points
        frames90[3] = (EMPTY, cloud(rng, 40), cloud(rng, 20))        # an empty corner, surf, outlier cloud, an empty frame
        frames90[5] = (cloud(rng, 30), EMPTY, cloud(rng, 20))
        frames90[6] = (cloud(rng, 30), cloud(rng, 40), EMPTY)
        frames90[7] = (EMPTY, EMPTY, EMPTY)

        def exact(total):   # N = K + 3: frame 1 is the one droppable frame, the K + 1 frames behind it move: `total` points, behind one copy item that stays
            part = [total // (K + 1) + (1 if i < total % (K + 1) else 0) for i in range(K + 1)]
            return [cloud(rng, ITEM), cloud(rng, 31)] + [cloud(rng, m) for m in part]

        dup40 = {int(i): int(rng.integers(0, i)) for i in rng.choice(np.arange(1, 35), 14, replace=False)}
        ends = sorted(dup40)[:3]                                     # loop edges whose endpoints would otherwise be dropped
        # (slot, replica, clouds, poses, loop edges (a, b), what)
        setups = [
            (3, 96, rand_clouds(rng, 1, 90), line_poses(rng, 1), [], "N = 1"),
            (10, 97, rand_clouds(rng, K, 90), line_poses(rng, K, {1: 0}), [], "N = K"),
            (20, 98, rand_clouds(rng, K + 1, 90), line_poses(rng, K + 1, {2: 0}), [], "N = K + 1"),
            (40, 99, rand_clouds(rng, K + 2, 90), line_poses(rng, K + 2, {1: 0}), [], "N = K + 2: every frame is protected"),
            (60, 100, rand_clouds(rng, 2 * K + 3, 90), line_poses(rng, 2 * K + 3, {1: 0}), [], "N = 2 K + 3, the first drop at frame 1"),
            (63, 101, rand_clouds(rng, 2 * K + 3, 90), line_poses(rng, 2 * K + 3, {5: 2}), "closed", "N = 2 K + 3, the first drop late, loop_closed_ cleared by an applied optimise"),
            (64, 102, rand_clouds(rng, 2 * K + 3, 90), line_poses(rng, 2 * K + 3, {i: 0 for i in range(1, 2 * K + 3)}), [(3, 9)], "N = 2 K + 3 at one place: everything droppable dropped"),
            (70, 103, rand_clouds(rng, 40, 90), line_poses(rng, 40, dup40), [(ends[0], 38), (39, ends[1]), (ends[2], ends[0])], "N = 40, loop edges at frames that would be dropped"),
            (90, 104, frames90, line_poses(rng, 12, {1: 0, 4: 2}), [(6, 0)], "a frame of three copy items + 37 points, empty clouds, an empty frame"),
            (91, 105, exact(ITEM), line_poses(rng, K + 3, {1: 0}), [], "moved points exactly one copy item, kept points exactly two"),
            (92, 106, exact(ITEM + 1), line_poses(rng, K + 3, {1: 0}), [], "one more"),
            (93, 107, exact(ITEM - 1), line_poses(rng, K + 3, {1: 0}), [], "one less"),
            (127, 108, exact(2 * ITEM), line_poses(rng, K + 3, {1: 0}), [], "two copy items, the last slot"),
        ]
        for s, rep, cl, po, loops, what in setups:
            n = len(po)
            add(h, s, cl, po, stamps=np.arange(n) * 7.5 + s)
            if loops == "closed":   # a loop edge that agrees with the poses to a few centimetres; the applied optimise clears loop_closed_
                X = R.from_pose6(po)
                h.graph_add_edge(n - 1, 0, R.compose(R.between(X[n - 1], X[0]), rigid([0, 0, 0.01], [0.05, 0.02, 0])[:3]), np.full(6, 1e-2), slot=s)
                g = h.graph_optimize([s], apply=True)[0]
                assert g["status"] == 2 and g["applied"] == 1 and h.graph_status(s)[2] == 0, g
            else:
                for a, b in loops:
                    loop_edge(h, s, a, b, rng)
        slots = [s for s, *_ in setups]
        assert min(slots) < 64 <= max(slots), "both stream groups"
        g = h.graph_optimize(slots)      # an estimate that the thin has to discard
        assert all(h.graph_status(s)[3] == h.map_status(s)[0] for s, r in zip(slots, g) if r["status"] >= 1) and sum(r["status"] >= 1 for r in g) >= 8, g
        for s in (5, 77):                # bystanders in both groups
            add(h, s, rand_clouds(rng, 7, 60), line_poses(rng, 7, {1: 0}))
        keeps = {s: expected_keep(h, s, MIN_DIST) for s in slots}
        first = {s: int(np.argmin(keeps[s])) if (keeps[s] == 0).any() else len(keeps[s]) for s in slots}
        assert first[60] == 1 and first[63] == 5 and keeps[64].tolist() == [1, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1] and first[90] == 1 and keeps[90][4] == 0
        assert all(keeps[70][e] == 1 for e in ends) and int((keeps[70] == 0).sum()) == 11, keeps[70]
        for s, rep, *_ in setups:
            if (keeps[s] == 0).any():
                host_thin(h, s, rep, keeps[s])
        before = {s: snap(h, s) for s in slots + [5, 77, 0, 126]}
        res = h.map_thin(slots[::-1], MIN_DIST)[::-1]    # (listed in descending order: a slot's result does not depend on the order)
        for (s, rep, cl, po, loops, what), r in zip(setups, res):
            nb, pb = len(keeps[s]), int(dict(before[s])["map_status"][2])
            if (keeps[s] == 0).any():
                assert (r["status"], r["frames_before"], r["frames"], r["points_before"]) == (2, nb, int(keeps[s].sum()), pb), (what, r)
                assert h.map_status(s)[:3] == h.map_status(rep)[:3] == (r["frames"], 0, r["points"]), (what, r)
                check_thinned(h, s, rep, before[s], what)
            else:
                assert r == dict(status=1, frames_before=nb, frames=nb, points_before=pb, points=pb), (what, r)
                same(before[s], snap(h, s), f"{what}: nothing to drop, slot {s} is byte-unchanged")
        assert [res[slots.index(s)]["points"] for s in (91, 92, 93)] == [2 * ITEM, 2 * ITEM + 1, 2 * ITEM - 1], "kept and moved points at a multiple of the copy item, one more, one less"
        assert res[slots.index(90)]["frames"] == 10
        for s in (5, 77, 0, 126):
            same(before[s], snap(h, s), f"a slot that is not in the call: {s}")
        # an optimise on both
        thinned = [(s, rep) for s, rep, *_ in setups if (keeps[s] == 0).any()]
        ga, gb = h.graph_optimize([s for s, _ in thinned]), h.graph_optimize([r for _, r in thinned])
        for (s, rep), a, b in zip(thinned, ga, gb):
            for key in a:
                assert_bit_equal(np.asarray(a[key]), np.asarray(b[key]), f"optimise of slot {s} and its replica: {key}")
            n = h.graph_status(s)[3]
            assert n == h.graph_status(rep)[3]
            assert_bit_equal(h.graph_get_estimate(n=n, slot=s), h.graph_get_estimate(n=n, slot=rep), f"estimate of slot {s} and its replica")
        # a second thin of a thinned slot: nothing is left to drop at the same distance
        again = h.map_thin([60, 70], MIN_DIST)
        assert [r["status"] for r in again] == [1, 1], again
        # the thinned slot takes further frames like its replica: id N', a chain edge from frame N' - 1
        for s, rep in ((64, 102), (90, 104)):
            cl, po = rand_clouds(rng, 2, 50), line_poses(rng, 2) + np.array([200, 5, 0, 0, 0, 0], F32)
            for slot in (s, rep):
                add(h, slot, cl, po)
            same(snap_vs_replica(h, s), snap_vs_replica(h, rep), f"two more frames on the thinned slot {s} and its replica")
    finally:
        h.close()


@pytest.mark.gpu
def test_untouched_slots_and_argument_errors():
    """status 1 (nothing to drop, min_dist 0 or negative), 0 (no key frame) and -1 (the archive dropped frames) leave the slot byte-unchanged while
    another slot of the call is thinned; every ALEGO_ERR_ARG case leaves all slots untouched"""
    rng = np.random.default_rng(67)
    MAXF = 8
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=8)
    h.map_enable(MAXF, 4000)
    h.graph_enable(4, ODOM_VAR)
    try:
        add(h, 0, rand_clouds(rng, K + 1, 60), line_poses(rng, K + 1, {1: 0}))          # every frame protected
        add(h, 2, rand_clouds(rng, MAXF + 1, 60), line_poses(rng, MAXF + 1, {1: 0}))    # dropped frames
        assert h.map_status(2)[1] == 1
        for s in (3, 5, 6):
            add(h, s, rand_clouds(rng, MAXF, 60), line_poses(rng, MAXF, {1: 0, 2: 0}))
        loop_edge(h, 3, 2, 6, rng)
        keep = expected_keep(h, 3, MIN_DIST)
        assert keep.tolist() == [1, 0, 1, 1, 1, 1, 1, 1]
        host_thin(h, 3, 4, keep)
        every = {s: snap(h, s) for s in range(8)}
        res = h.map_thin([0, 1, 2, 3], MIN_DIST)
        assert [r["status"] for r in res] == [1, 0, -1, 2], res
        assert res[1] == dict(status=0, frames_before=0, frames=0, points_before=0, points=0) and res[2]["frames"] == res[2]["frames_before"] == MAXF
        for s in (0, 1, 2, 5, 6, 7):
            same(every[s], snap(h, s), f"slot {s} (status 1 / 0 / -1 or not listed) is byte-unchanged")
        check_thinned(h, 3, 4, every[3], "status 2 next to the untouched slots")
        for md in (0.0, -1.0):
            assert [r["status"] for r in h.map_thin([5, 6], md)] == [1, 1]
        every = {s: snap(h, s) for s in range(8)}
        for slots, md in (([8], 1.0), ([-1], 1.0), ([5, 6, 5], 1.0), ([5], float("nan")), ([5], float("inf")), ([5, 6], -float("inf"))):
            with pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_ARG}\)"):
                h.map_thin(slots, md)
        for s in range(8):
            same(every[s], snap(h, s), f"ALEGO_ERR_ARG: slot {s}")
        assert h.map_thin([], 1.0) == []
    finally:
        h.close()
    h = binding.Handle(_params(False), n_slots=2)
    try:
        with pytest.raises(binding.AlegoError, match="the key-frame archive is off"):
            h.map_thin([0], 1.0)
        h.loc_enable([(np.zeros(6, F32), EMPTY, EMPTY, EMPTY)], 0.0)
        with pytest.raises(binding.AlegoError, match="not available on a localising handle"):
            h.map_thin([0], 1.0)
    finally:
        h.close()


@pytest.mark.gpu
def test_thin_with_the_graph_off_and_regained_capacity():
    """an archive filled to max_keyframes exactly (a further frame would be dropped, as on the untouched copy in slot 2): after the thin the next
    frames are stored, and the slot goes on like its replica; the key-pose graph is off"""
    rng = np.random.default_rng(71)
    MAXF = 12
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=4)
    h.map_enable(MAXF, MAXF * 60)
    try:
        cl, po = rand_clouds(rng, MAXF, 60), line_poses(rng, MAXF, {1: 0, 3: 2, 4: 2, 6: 5})
        for s in (0, 2):
            add(h, s, cl, po, stamps=np.arange(MAXF) * 2.5)
        assert h.map_status(0)[:3] == (MAXF, 0, MAXF * 60), "full: frames and points exactly at capacity"
        keep = expected_keep(h, 0, MIN_DIST)
        assert int(keep.sum()) == MAXF - 4
        host_thin(h, 0, 1, keep)
        before = snap(h, 0)
        r = h.map_thin([0], MIN_DIST)[0]
        assert r == dict(status=2, frames_before=MAXF, frames=MAXF - 4, points_before=MAXF * 60, points=(MAXF - 4) * 60), r
        check_thinned(h, 0, 1, before, "graph off")
        more, mpo = rand_clouds(rng, 3, 60), line_poses(rng, 3) + np.array([100, 0, 0, 0, 0, 0], F32)
        for s in (0, 1, 2):
            add(h, s, more, mpo)
        assert h.map_status(0)[:3] == (MAXF - 1, 0, (MAXF - 1) * 60), "room regained: the next frames are stored"
        assert h.map_status(2)[:2] == (MAXF, 3), "the full archive drops them"
        assert h.map_thin([2], MIN_DIST)[0]["status"] == -1
        same(snap_vs_replica(h, 0), snap_vs_replica(h, 1), "three more frames after the thin")
    finally:
        h.close()


@pytest.mark.gpu
def test_descriptors_after_a_thin():
    """an appearance search before the thin describes every frame; the thin keeps the descriptors below the first dropped frame; the search after
    it describes the rest again: descriptors and results equal those of the replica"""
    rng = np.random.default_rng(73)
    n = 2 * K + 6
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=4)
    h.map_enable(32, 1 << 14)
    h.graph_enable(4, ODOM_VAR)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    try:
        add(h, 0, rand_clouds(rng, n), line_poses(rng, n, {4: 1, 6: 3}), stamps=np.arange(n) * 40.0)
        h.loop_search_appearance([0], verify=0)
        assert h.debug_get("la_desc", slot=0).size == 1200 * n
        old = h.debug_get("la_desc", slot=0).reshape(n, 1200).copy()
        keep = expected_keep(h, 0, MIN_DIST)
        assert keep.tolist() == [1, 1, 1, 1, 0, 1, 0] + [1] * (n - 7)
        host_thin(h, 0, 1, keep)
        before = snap(h, 0)
        assert h.map_thin([0], MIN_DIST)[0]["status"] == 2
        assert_bit_equal(h.debug_get("la_desc", slot=0).reshape(-1, 1200), old[:4], "the descriptors below the first dropped frame stay")
        x, y = h.loop_search_appearance([0, 1], verify=0)
        for key in sorted(x):
            assert_bit_equal(np.asarray(x[key]), np.asarray(y[key]), f"appearance search on the thinned slot and its replica: {key}")
        for name in ("la_desc", "la_key"):
            assert_bit_equal(h.debug_get(name, slot=0), h.debug_get(name, slot=1), f"{name} of the thinned slot and its replica")
        assert_bit_equal(h.debug_get("la_desc", slot=0).reshape(-1, 1200), old[keep != 0], "a kept frame's descriptor depends on its clouds only")
        check_thinned(h, 0, 1, before, "descriptors")
    finally:
        h.close()


@pytest.mark.gpu
def test_the_live_stream_continues_after_a_thin():
    """Two slots replay the same synthetic stream until 2 K + 3 key frames exist.  Slot A is thinned, slot B gets alego_lm_reset_window; both go on
    for 30 scans.  The window refills from the newest K frames, which are protected: A's odometry and map poses equal B's bit for bit at every
    scan, A saves key frames at the same scans as B with equal clouds and poses, ids lower by the number dropped, chain edges equal up to that shift."""
    p = _params(False, recent_keyframe_num=K)
    A, B = 0, 1
    h = binding.Handle(p, n_slots=2)
    h.map_enable(64, 1 << 19)
    h.graph_enable(4)
    try:
        k = 0
        while h.lm_keyframe_count(slot=A) < 2 * K + 3:
            for s in (A, B):
                h.scan_process(_scan(p, k), stages=7, slot=s, stamp=0.1 * k)
            k += 1
            assert k < 400, "the synthetic stream saves a key frame every few scans"
        n = h.lm_keyframe_count(slot=B)
        assert n == 2 * K + 3 == h.map_status(A)[0]
        po = archived_poses(h, A)
        assert_bit_equal(po, archived_poses(h, B), "the same stream")
        md = 1.25 * float(np.linalg.norm(po[1, :3].astype(np.float64) - po[0, :3]))    # frame 1 lies closer than this to frame 0
        keep = expected_keep(h, A, md)
        dropped = int((keep == 0).sum())
        assert dropped >= 1 and keep[1] == 0, keep
        state = h.debug_get("lm_state", slot=A)
        r = h.map_thin([A], md)[0]
        assert (r["status"], r["frames"]) == (2, n - dropped), r
        h.lm_reset_window(slot=B)
        assert_bit_equal(h.debug_get("lm_state", slot=A), state, "map -> odom and params_ are untouched")
        saved = 0
        for j in range(30):
            out = [h.scan_process(_scan(p, k + j), stages=7, slot=s, stamp=0.1 * (k + j)) for s in (A, B)]
            assert out[0][0] == out[1][0], (j, out[0][0], out[1][0])
            for a, b, what in ((out[0][1], out[1][1], "odometry"), (out[0][2], out[1][2], "map pose")):
                for key in ("t", "q", "params"):
                    assert_bit_equal(a[key], b[key], f"scan {j} after the thin: {what} {key}")
            na, nb = h.lm_keyframe_count(slot=A), h.lm_keyframe_count(slot=B)
            assert na == nb - dropped, (j, na, nb)
            if out[0][0] & binding.FLAG_LM_KEYFRAME:
                saved += 1
                fa, fb = h.lm_get_keyframe(na - 1, slot=A), h.lm_get_keyframe(nb - 1, slot=B)
                for key in ("pose", "corner", "surf", "outlier"):
                    assert_bit_equal(fa[key], fb[key], f"scan {j}: the key frame saved after the thin: {key}")
        assert saved >= 2, saved
        na, nb = h.map_status(A)[0], h.map_status(B)[0]
        assert (na, h.map_status(A)[1]) == (nb - dropped, 0)
        ea, eb = h.graph_get_edges(kind=0, first=n - dropped, slot=A), h.graph_get_edges(kind=0, first=n, slot=B)
        assert ea["frm"].tolist() == (eb["frm"] - dropped).tolist() and ea["to"].tolist() == (eb["to"] - dropped).tolist() and len(ea["frm"]) == saved
        assert_bit_equal(ea["between"], eb["between"], "chain edges of the frames saved after the thin")
        assert_bit_equal(ea["variance"], eb["variance"], "their variances")
        for f in range(n - dropped, na):
            x, y = h.map_get_keyframe(f, slot=A), h.map_get_keyframe(f + dropped, slot=B)
            for key in ("pose", "corner", "surf", "outlier"):
                assert_bit_equal(x[key], y[key], f"archived frame {f} of the thinned slot: {key}")
        assert_bit_equal(h.map_get_stamps(slot=A)[n - dropped:], h.map_get_stamps(slot=B)[n:], "stamps of the frames saved after the thin")
    finally:
        h.close()


@pytest.mark.gpu
def test_replay_thin_agrees_with_the_binding(tmp_path):
    """examples/replay 150 --recent-keyframes K --align 30 --merge --thin D: the align, merge and thin lines equal what the binding's calls give;
    --save-map holds the thinned map.  (With the default recent_keyframe_num of 50 the 28 frames of this union would all be resident and stay.)"""
    n, start2, D = 150, 30, 1.5
    exe = os.path.join(ROOT, "examples", "replay")
    out = subprocess.run([exe, str(n), "--recent-keyframes", str(K), "--align", str(start2), "--merge", "--thin", str(D), "--save-map", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith(("align:", "merge:", "thin:"))]
    p = synth.default_params(16, 1800)
    p.recent_keyframe_num = K
    h = binding.Handle(p, n_slots=2)
    try:
        h.map_enable(4096, 1 << 24)
        h.graph_enable(binding.ALIGN_MAX_QUERIES)
        h.loop_appearance_enable()
        for k in range(n):
            h.scan_process(_scan(p, k), stages=7, slot=0, stamp=0.1 * k)
            h.scan_process(_scan(p, start2 + k), stages=7, slot=1, stamp=0.1 * k)
        r = h.map_align([(1, 0)])[0]
        assert r["status"] == 2
        m = h.map_merge([(1, 0)], r["T"], seam_variance=SEAM, hyps=[r["hyp"]])[0]
        g = h.graph_optimize([0], apply=True)[0]
        t = h.map_thin([0], D)[0]
        want = [f"align: status {r['status']} queries {r['n_queries']} accepted {r['n_accepted']} support {r['support']} T" + "".join(f" {v:.9g}" for v in np.asarray(r["T"]).reshape(12)),
                f"merge: status {m['status']} frames {m['frames']} points {m['points']} loop_edges {m['loop_edges']} cross_edges {m['cross_edges']} optimise status {g['status']} "
                f"poses {g['n_poses']} loops {g['n_loops']} iterations {g['iterations']} cost {g['cost0']:.9g} -> {g['cost']:.9g}",
                f"thin: status {t['status']} frames {t['frames_before']} -> {t['frames']} points {t['points_before']} -> {t['points']}"]
        print("\n".join(got))
        assert got == want, (got, want)
        assert t["status"] == 2 and t["frames"] < t["frames_before"] == g["n_poses"] and t["points"] < t["points_before"], t
        hdr = open(os.path.join(str(tmp_path), "keypose.pcd"), "rb").read(400).decode(errors="replace")
        assert f"POINTS {t['frames']}" in hdr and h.map_status(0)[0] == t["frames"], hdr
    finally:
        h.close()
