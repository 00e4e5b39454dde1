"""Relocalisation in the frozen map (alego_reloc_enable / alego_loc_relocalize, kernels_reloc.hip): slots of a
localising handle are placed without an initial pose.

The rule (csrc/reloc_math.h) is restated in numpy f32 with the same operation order; the sector uses this host's libm atan2f
(oracle_libm_atan2f_array), to which test_gpu_parity pins the device's d_atan2f.  The search is compared with a numpy brute force over
all frames and all 60 shifts.  Verification is emulated with the UNCHANGED oracle's loop_icp: the query's three clouds as the frame
(guess6, corner, surf, outlier), the map frames around the candidate as its history.

Clouds with non-finite coordinates reach the device rule as KEY FRAMES (alego_loc_enable stores a frame's raw clouds as they are, and
rl_desc reads those) and the host twin; they are not fed as scan clouds: there LaserMapping's VoxelGrid comes first, whose input the
front end keeps finite, so laser_*_ds_ never holds such a point.

Ground truth: stream s is the lap's trajectory 70 s scans ahead (csrc/synth.cpp); the map frame is the world frame moved to synth.pose(0).
A scan rotated about z by a is the scan of a sensor whose yaw is a less.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAP = 560
NS, NR = 60, 20
LI_RUN, LI_OPTIMIZED = 2, 11   # (lm_ctx.h)
LD_T_M2L, LD_Q_M2L = 20, 23
MAX_RANGE, Z_OFFSET = 40.0, 4.0   # on the lap (the values of the CPU prototype)
NEW_SYMBOLS = ["alego_reloc_enable", "alego_loc_relocalize", "alego_reloc_descriptor", "alego_reloc_match", "alego_debug_reloc_search"]
# (stream, k0, rotation of the scan about z): scans k0, k0 + 1 go to a fresh instance
QUERIES = [(1, 5, 1.0), (2, 40, 2.5), (3, 100, -0.8), (4, 11, 3.1), (5, 300, 0.05), (6, 130, -2.2), (3, 190, 0.0), (2, 333, 0.0)]
POS_TOL, ANG_TOL = 0.25, 0.02   # the premise: the right place was found (the prototype measured 0.075 m / 0.0044 rad at worst)
EMPTY = np.zeros((0, 4), F32)


def _O():
    from oracle import oracle_py
    return oracle_py


# ---- the rule in numpy ----------------------------------------------------------------------------------------------------------
def _atan2f(y, x):
    y, x = np.ascontiguousarray(y, F32), np.ascontiguousarray(x, F32)
    out = np.empty_like(y)
    if y.size:
        _O().lib().oracle_libm_atan2f_array(y.ctypes.data, x.ctypes.data, out.ctypes.data, y.size)
    return out


def desc_np(pts, max_range, z_offset):
    """(descriptor (60, 20) u8, ring key (20,) u16)"""
    p = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    mr = F32(max_range if max_range > 0 else 80.0)
    zo = F32(z_offset if np.isfinite(z_offset) else 4.0)
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        w = mr / F32(20.0)
        r = np.sqrt((x * x) + (y * y))
        fr = np.floor(r / w)
        ok &= fr < F32(20.0)
        fs = np.floor((_atan2f(y, x) + F32(np.pi)) * F32(60.0 / (2.0 * np.pi)))
        fc = np.minimum(F32(255.0), np.maximum(F32(1.0), np.floor((z + zo) * F32(16.0)) + F32(1.0)))
        assert r.dtype == F32 and fr.dtype == F32 and fs.dtype == F32 and fc.dtype == F32
    D = np.zeros((NS, NR), np.int64)
    sector = np.minimum(59, fs[ok]).astype(np.int64)
    np.maximum.at(D, (sector, fr[ok].astype(np.int64)), fc[ok].astype(np.int64))
    return D.astype(np.uint8), D.sum(axis=0).astype(np.uint16)


def match_all_np(M, Q):
    """(D_i, s_i) of query Q (60, 20) against every frame of M (N, 60, 20): the brute force over all 60 shifts"""
    M = np.ascontiguousarray(M, np.uint8).reshape(-1, NS, NR)
    Q = np.ascontiguousarray(Q, np.uint8).reshape(NS, NR)
    best = np.full(M.shape[0], 1 << 40, np.int64)
    shift = np.zeros(M.shape[0], np.int64)
    for s in range(NS):
        Qs = np.roll(Q, -s, axis=0)[None]   # Qs[c] = Q[(c + s) mod 60]
        d = (np.maximum(M, Qs) - np.minimum(M, Qs)).reshape(M.shape[0], -1).sum(axis=1, dtype=np.int64)
        upd = d < best
        best[upd], shift[upd] = d[upd], s
    return best, shift


def search_np(M, Qs, n_cand):
    """ids, dists, shifts (n_q, n_cand), -1 where the map has fewer frames: the n_cand smallest in the order (D, id)"""
    M = np.ascontiguousarray(M, np.uint8).reshape(-1, NS, NR)
    Qs = np.ascontiguousarray(Qs, np.uint8).reshape(-1, NS, NR)
    ids, dists, shifts = (np.full((Qs.shape[0], n_cand), -1, np.int32) for _ in range(3))
    for q in range(Qs.shape[0]):
        d, s = match_all_np(M, Qs[q])
        order = np.lexsort((np.arange(len(d)), d))[:n_cand]
        ids[q, :len(order)], dists[q, :len(order)], shifts[q, :len(order)] = order, d[order], s[order]
    return ids, dists, shifts


def _pts(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.c_[xyz, np.zeros(len(xyz))].astype(F32)


def _rounding_range():
    """a max_range whose ring width w has a radius r < max_range with r / w rounding UP to 20.0f: the point is skipped"""
    for mr in np.arange(30.0, 32.0, 0.001):
        mr = F32(mr)
        w = mr / F32(20.0)
        r = np.nextafter(mr, F32(0))
        if r < mr and F32(r / w) == F32(20.0):
            return float(mr), float(r)
    raise AssertionError("no such range")


def constructed_clouds():
    """(name, cloud, max_range, z_offset); every cloud is finite unless its name says otherwise"""
    w = MAX_RANGE / 20.0
    out = []
    ring_edges = [[k * w, 0, 0.5] for k in range(0, 21)] + [[0, -k * w, -1.0] for k in range(1, 21)] + [[-k * w, 0, 2.0] for k in range(1, 21)]
    out.append(("r at exact multiples of w", _pts(ring_edges), MAX_RANGE, Z_OFFSET))
    below = float(np.nextafter(F32(MAX_RANGE), F32(0)))
    out.append(("just below and at max_range", _pts([[below, 0, 0], [MAX_RANGE, 0, 0], [0, below, 1], [0, -MAX_RANGE, 1], [24, 32, 0], [-24.0, float(np.nextafter(F32(32), F32(0))), 0]]), MAX_RANGE, Z_OFFSET))
    mr, r = _rounding_range()
    out.append(("r / w rounds up to 20", _pts([[r, 0, 0], [0, r, 0], [float(np.nextafter(F32(r), F32(0))), 0, 3], [1, 1, 1]]), mr, Z_OFFSET))
    out.append(("azimuth +-pi and the origin", _pts([[-1, 0.0, 0], [-1, -0.0, 1], [-3, 1e-30, 0], [-3, -1e-30, 2], [0, 0, 0], [0.0, -0.0, 1], [5, 0, 0], [5, -1e-7, 0], [0, 7, 0], [0, -7, 0]]), MAX_RANGE, Z_OFFSET))
    zs = [-100.0, -4.0 - 1e-3, -4.0, -4.0 + 1 / 16, -4.0 + 1 / 16 - 1e-6, 11.8125, 11.875, 11.875 - 1e-5, 12.0, 50.0]
    out.append(("z at both clamps", _pts([[3 + 2.5 * i, 1, z] for i, z in enumerate(zs)]), MAX_RANGE, Z_OFFSET))
    out.append(("default range and offset", _pts([[79.9, 0, 0], [80.0, 0, 0], [10, 10, -3.99], [-50, 20, 7]]), 0.0, float("nan")))
    out.append(("empty", EMPTY, MAX_RANGE, Z_OFFSET))
    nf = np.array([[np.nan, 1, 1, 0], [1, np.nan, 1, 0], [1, 1, np.nan, 0], [np.inf, 1, 1, 0], [1, -np.inf, 1, 0], [1, 1, np.inf, 0], [1, 1, -np.inf, 0], [2, 2, 2, 0],
                   [1e30, 1e30, 0, 0], [3e38, 3e38, 0, 0]], F32)
    out.append(("non-finite: NaN and +-inf coordinates", nf, MAX_RANGE, Z_OFFSET))
    rng = np.random.default_rng(3)
    out.append(("random", np.c_[rng.uniform(-45, 45, (4000, 2)), rng.uniform(-6, 14, 4000), np.zeros(4000)].astype(F32), MAX_RANGE, Z_OFFSET))
    return out


def match_cases():
    """(name, Q, M) descriptors (60, 20) u8"""
    rng = np.random.default_rng(11)
    rnd = lambda: rng.integers(0, 256, (NS, NR)).astype(np.uint8)
    sparse = lambda: (rnd() * (rng.random((NS, NR)) < 0.3)).astype(np.uint8)
    out = [(f"random {i}", rnd(), rnd()) for i in range(3)] + [(f"sparse {i}", sparse(), sparse()) for i in range(3)]
    const = np.repeat(rng.integers(0, 256, (1, NR)), NS, axis=0).astype(np.uint8)
    out.append(("constant across sectors: every shift ties, s = 0", const, np.repeat(rng.integers(0, 256, (1, NR)), NS, axis=0).astype(np.uint8)))
    a = sparse()
    out.append(("best shift 59", a, np.roll(a, -59, axis=0)))   # M[c] = Q[(c + 59) mod 60]
    out.append(("best shift 1", a, np.roll(a, -1, axis=0)))
    out.append(("all-zero query", np.zeros((NS, NR), np.uint8), rnd()))
    out.append(("identical: D = 0", a, a.copy()))
    return out


def _yaw_R(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def rotated_scan(p, stream, k, ang):
    pts = synth.scan(p, k, stream)
    if ang != 0.0:
        xy = pts[:, :2].astype(np.float64) @ _yaw_R(ang)[:2, :2].T
        pts = np.c_[xy, pts[:, 2:]].astype(F32)
    return pts


def truth_in_map(stream, k, ang):
    """(position, rotation) of the sensor of scan k of `stream`, its points rotated about z by ang, in the map frame"""
    g, g0 = synth.pose(k, stream), synth.pose(0, 0)
    assert g0[3] == 0.0
    return g[:3] - g0[:3], _yaw_R(g[3] - ang)


def pose_error(t_map, stream, k, ang):
    t, R = truth_in_map(stream, k, ang)
    T = np.asarray(t_map, np.float64).reshape(4, 4)
    c = (np.trace(R.T @ T[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(T[:3, 3] - t)), float(np.arccos(np.clip(c, -1.0, 1.0)))


def guess_of(kp, i, s):
    g = np.array(kp[i], F32)
    g[5] = g[5] - F32(s) * F32(2.0 * np.pi / 60.0)
    return g


def emulate_verify(p, frames, kp, clouds, i, s):
    """the oracle's loop_icp on candidate (i, s): (result, guess6, t_map)"""
    g = guess_of(kp, i, s)
    fr = [(g,) + tuple(clouds)]
    for j in range(i - p.lc_search_num, i + p.lc_search_num + 1):
        if 0 <= j < len(frames):
            fr.append((kp[j], frames[j]["corner"], frames[j]["surf"], frames[j]["outlier"]))
    want, _ = _O().loop_icp(p, fr)
    t_map, _ = binding.loop_constraint(want["T"], g, g)
    return want, g, np.asarray(t_map, F32).reshape(4, 4)


def map_descriptors(frames):
    return np.array([desc_np(np.concatenate([f["corner"], f["surf"], f["outlier"]]), MAX_RANGE, Z_OFFSET)[0] for f in frames])


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_relocalisation_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s
    assert "ALEGO_RELOC_MAX_CAND 8" in hdr and binding.RELOC_MAX_CAND == 8


@pytest.fixture(scope="module")
def oracle_lap():
    """the lap mapped by the oracle: its key frames and key poses"""
    O = _O()
    p = synth.default_params(16, 1800)
    o = O.Oracle(p)
    for k in range(LAP):
        o.process_scan(synth.scan(p, k))
    kp = o.get("lm_keyposes").reshape(-1, 6).astype(F32)
    frames = []
    for i in range(len(kp)):
        c, s, ol = o.lm_keyframe(i)
        frames.append(dict(pose=kp[i], corner=c, surf=s, outlier=ol))
    o.close()
    assert len(frames) >= 40
    return dict(p=p, frames=frames, kp=kp, desc=map_descriptors(frames))


def test_descriptor_twin_equals_numpy(oracle_lap):
    cases = constructed_clouds()
    f = oracle_lap["frames"][17]
    cases.append(("a key frame of the lap", np.concatenate([f["corner"], f["surf"], f["outlier"]]), MAX_RANGE, Z_OFFSET))
    for name, pts, mr, zo in cases:
        d, k = binding.reloc_descriptor(pts, mr, zo)
        wd, wk = desc_np(pts, mr, zo)
        assert np.array_equal(d, wd), (name, np.argwhere(d != wd)[:5])
        assert np.array_equal(k, wk), name
        assert np.array_equal(k, d.astype(np.int64).sum(axis=0)), name
    # what the constructed clouds are there for
    by = {c[0]: binding.reloc_descriptor(c[1], c[2], c[3])[0] for c in cases}
    edges = by["r at exact multiples of w"]
    assert all(edges[30, k] > 0 for k in range(20)) and edges.sum(axis=0).astype(bool).all(), "r = k w lies in ring k; r = 20 w is skipped"
    assert np.count_nonzero(by["just below and at max_range"]) == 2 and by["just below and at max_range"][:, 19].astype(bool).sum() == 2, "the two points just below stay"
    assert np.count_nonzero(by["r / w rounds up to 20"]) == 2, "the two points whose quotient rounds up to 20 are skipped"
    az = by["azimuth +-pi and the origin"]
    assert az[0].any() and az[59].any() and az[30].any() and az[15].any() and az[45].any(), "-pi -> sector 0, +pi -> 59 (clamped), 0 -> 30, -pi/2 -> 15, pi/2 -> 45"
    zc = by["z at both clamps"]
    assert zc.max() == 255 and zc[zc > 0].min() == 1
    assert np.count_nonzero(by["non-finite: NaN and +-inf coordinates"]) == 1
    assert not by["empty"].any()
    assert np.count_nonzero(by["a key frame of the lap"]) > 100


def test_match_twin_equals_numpy():
    for name, Q, M in match_cases():
        got = binding.reloc_match(Q, M)
        d, s = match_all_np(M[None], Q)
        assert got == (int(d[0]), int(s[0])), (name, got, d, s)
        per_shift = [int(np.abs(np.roll(Q, -k, axis=0).astype(np.int64) - M).sum()) for k in range(NS)]
        assert got[0] == min(per_shift) and got[1] == per_shift.index(min(per_shift)), name
        if name.startswith("constant"):
            assert got[1] == 0 and len(set(per_shift)) == 1
        if name.startswith("best shift 59"):
            assert got == (0, 59)
        if name.startswith("identical"):
            assert got == (0, 0)
    # the bound the search prunes with
    rng = np.random.default_rng(5)
    for _ in range(20):
        Q, M = (rng.integers(0, 256, (NS, NR)).astype(np.uint8) for _ in range(2))
        B = int(np.abs(Q.astype(np.int64).sum(axis=0) - M.astype(np.int64).sum(axis=0)).sum())
        assert B <= binding.reloc_match(Q, M)[0]


def oracle_query(p, stream, k0, ang):
    """the three down-sampled clouds of the last mapping frame of a fresh oracle fed scans k0, k0 + 1"""
    o = _O().Oracle(p)
    for k in (k0, k0 + 1):
        o.process_scan(rotated_scan(p, stream, k, ang))
    clouds = (o.get("lm_corner_ds"), o.get("lm_surf_ds"), o.get("lm_outlier_ds"))
    o.close()
    return clouds


def test_the_premise_on_the_reference_side(oracle_lap):
    """numpy search + the oracle's loop_icp on the oracle-mapped lap: every query is accepted at the right place"""
    p, frames, kp = oracle_lap["p"], oracle_lap["frames"], oracle_lap["kp"]
    for stream, k0, ang in QUERIES:
        clouds = oracle_query(p, stream, k0, ang)
        Q, _ = desc_np(np.concatenate(clouds), MAX_RANGE, Z_OFFSET)
        ids, dists, shifts = search_np(oracle_lap["desc"], Q[None], 2)
        want, g, t_map = emulate_verify(p, frames, kp, clouds, int(ids[0, 0]), int(shifts[0, 0]))
        dp, da = pose_error(t_map, stream, k0 + 1, ang)
        print(f"query {(stream, k0, ang)}: frame {ids[0, 0]} D {dists[0, 0]} (next {dists[0, 1]}) shift {shifts[0, 0]} iterations {want['iterations']} "
              f"fitness {want['fitness']:.4f} error {dp:.4f} m {da:.5f} rad")
        assert want["converged"] and want["fitness"] <= p.lc_fitness_max, (stream, k0, ang, want)
        assert dp < POS_TOL and da < ANG_TOL, (stream, k0, ang, dp, da)


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    p = synth.default_params(16, 1800)
    for name, v in kw.items():
        setattr(p, name, v)
    return p


_SCANS = {}


def _scan(k):
    if k not in _SCANS:
        _SCANS[k] = synth.scan(_params(), k)
    return _SCANS[k]


@pytest.fixture(scope="module")
def lap_map():
    """the lap mapped once on a device SLAM handle with the archive on (as test_localize.py::lap_map)"""
    p = _params()
    h = binding.Handle(p)
    h.map_enable(256, 1 << 20)
    for k in range(LAP):
        h.scan_process(_scan(k), stages=7)
    nf, dropped = h.map_status()[:2]
    assert dropped == 0 and nf >= 40, (nf, dropped)
    frames = [h.map_get_keyframe(i) for i in range(nf)]
    h.close()
    kp = np.array([f["pose"] for f in frames], F32).reshape(-1, 6)
    return dict(frames=frames, kp=kp, desc=map_descriptors(frames))


def loc_handle(lap_map, n_slots, p=None, reloc=True, mr=MAX_RANGE, zo=Z_OFFSET):
    h = binding.Handle(p or _params(), n_slots=n_slots)
    h.loc_enable([(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in lap_map["frames"]], 0.0)
    if reloc:
        h.reloc_enable(mr, zo)
    return h


def feed_queries(h, queries, first_slot=0):
    for i, (stream, k0, ang) in enumerate(queries):
        for k in (k0, k0 + 1):
            flags = h.scan_process(rotated_scan(h.params, stream, k, ang), stages=7, slot=first_slot + i)[0]
            assert flags >= 0


def slot_clouds(h, slot):
    return tuple(h.debug_get(n, slot=slot) for n in ("lm_corner_ds", "lm_surf_ds", "lm_outlier_ds"))


def same_result(a, b):
    assert a.keys() == b.keys()
    for k in a:
        va, vb = np.asarray(a[k]), np.asarray(b[k])
        assert va.shape == vb.shape and va.tobytes() == vb.tobytes(), (k, a[k], b[k])


@pytest.fixture(scope="module")
def eight(lap_map):
    """the eight queries as eight unplaced slots of one handle, after their first mapping frame; relocalised with verify = 1, apply = 0"""
    h = loc_handle(lap_map, 8)
    feed_queries(h, QUERIES)
    res = h.loc_relocalize(list(range(8)), n_cand=4, verify=1, apply=False)
    yield dict(h=h, res=res)
    h.close()


def _finite(c):
    return np.isfinite(c[1][:, :3]).all()


@pytest.mark.gpu
def test_device_descriptors_are_the_numpy_rule(lap_map):
    # the lap's frames
    h = loc_handle(lap_map, 1)
    got = h.debug_get("rl_map_desc").reshape(-1, NS, NR)
    assert np.array_equal(got, lap_map["desc"]), np.argwhere(got != lap_map["desc"])[:5]
    keys = h.debug_get("rl_map_key").view(np.uint16).reshape(-1, NR)
    assert np.array_equal(keys, lap_map["desc"].astype(np.int64).sum(axis=1))
    h.close()
    # the constructed clouds as key frames (split over the three kinds) and as scan clouds, one handle per (max_range, z_offset)
    cases = constructed_clouds()
    split = lambda a: (a[0::3], a[1::3], a[2::3])
    for mr, zo in [(MAX_RANGE, Z_OFFSET), (_rounding_range()[0], Z_OFFSET), (0.0, float("nan"))]:
        group = [c for c in cases if c[2] == mr and (c[3] == zo or (np.isnan(zo) and np.isnan(c[3])))]
        assert group
        h = binding.Handle(_params(lm_every=1))
        far = np.array([1e4, 0, 0, 0, 0, 0], F32)   # off the slot's window: the scans below are down-sampled and not registered (section 14, rule 5)
        h.loc_enable([(far,) + split(c[1]) for c in group], 0.0)
        h.reloc_enable(mr, zo)
        got = h.debug_get("rl_map_desc").reshape(-1, NS, NR)
        for i, c in enumerate(group):
            assert np.array_equal(got[i], desc_np(c[1], mr, zo)[0]), ("key frame", c[0])
        for c in group:   # alego_lm_process feeds slot 0: every call is a mapping frame of its own
            if not _finite(c):
                continue   # (module docstring)
            corner, surf, outl = split(c[1])
            h.lm_process(corner, surf, outl, dict(t=[0, 0, 0], q=[1, 0, 0, 0]))
            res = h.loc_relocalize([0], verify=0)[0]
            ds = np.concatenate(slot_clouds(h, 0))
            wd, wk = desc_np(ds, mr, zo)
            assert np.array_equal(h.debug_get("rl_query_desc").reshape(NS, NR), wd), ("scan", c[0])
            assert np.array_equal(h.debug_get("rl_query_key").view(np.uint16), wk), ("scan", c[0])
            assert res["status"] == (1 if wd.any() else 0), (c[0], res["status"])
        h.close()
    assert sum(1 for c in cases) == sum(1 for mr, zo in [(MAX_RANGE, Z_OFFSET), (_rounding_range()[0], Z_OFFSET), (0.0, float("nan"))]
                                       for c in cases if c[2] == mr and (c[3] == zo or (np.isnan(zo) and np.isnan(c[3])))), "every cloud went to a handle"


def search_cases():
    """(name, map descriptors (N, 60, 20), queries (n_q, 60, 20), n_cand)"""
    rng = np.random.default_rng(23)
    rnd = lambda n: rng.integers(0, 256, (n, NS, NR)).astype(np.uint8)
    sparse = lambda n: (rnd(n) * (rng.random((n, NS, NR)) < 0.3)).astype(np.uint8)
    out = []
    base = sparse(6)
    out.append(("duplicate frames: the lowest id first", np.concatenate([base, base, base[::-1]]), np.roll(base[:3], 7, axis=1), 4))
    half = sparse(5)[:, :30]
    sym = np.concatenate([half, half], axis=1)   # period 30: shifts s and s + 30 tie
    out.append(("symmetric descriptors", sym, np.roll(sym[:2], -11, axis=1), 4))
    one = sparse(1)[0]
    perm = np.array([np.stack([np.roll(one[:, r], int(rng.integers(0, NS))) for r in range(NR)], axis=1) for _ in range(40)])   # same ring keys, different D
    out.append(("identical ring keys: the bound prunes nothing", perm, np.concatenate([one[None], perm[:1]]), 4))
    lev = rng.integers(0, 200, (30, 1, NR)).astype(np.uint8)
    flat = np.repeat(lev, NS, axis=1)
    flat = np.concatenate([flat, flat[:10], flat[5:15]])   # the bound is the distance; ties at the threshold
    out.append(("sector-constant frames: the bound is tight", flat, np.concatenate([flat[3:5], np.repeat(rng.integers(0, 200, (1, 1, NR)).astype(np.uint8), NS, axis=1)]), 4))
    out.append(("N = 1", sparse(1), sparse(2), 4))
    out.append(("N < n_cand", sparse(3), sparse(2), 8))
    out.append(("all-zero frames", np.zeros((20, NS, NR), np.uint8), np.concatenate([sparse(1), np.zeros((1, NS, NR), np.uint8)]), 4))
    m = sparse(300)
    out.append(("n_cand = 1", m, np.roll(m[[5, 250]], 3, axis=1), 1))
    out.append(("n_cand = 8", m, np.roll(m[[7, 100, 299]], -20, axis=1), 8))
    return out


@pytest.fixture(scope="module")
def plain_handle():
    h = binding.Handle(_params())
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(search_cases())))
def test_search_kernels_equal_the_brute_force(plain_handle, case):
    name, M, Q, n_cand = search_cases()[case]
    want = search_np(M, Q, n_cand)
    for brute in (0, 1):
        plain_handle.set_option("ALEGO_RL_BRUTE", brute)
        got = plain_handle.debug_reloc_search(M, Q, n_cand)
        for g, w, what in zip(got, want, ("ids", "dists", "shifts")):
            assert np.array_equal(g, w), (name, "brute" if brute else "pruned", what, g, w)
    plain_handle.set_option("ALEGO_RL_BRUTE", 0)
    if name.startswith("duplicate"):
        assert (np.diff(want[0], axis=1)[np.diff(want[1], axis=1) == 0] > 0).all() and (np.diff(want[1], axis=1) == 0).any()
    if name.startswith("identical ring keys"):
        plain_handle.debug_reloc_search(M, Q, n_cand)
        ev, total = plain_handle.debug_get("rl_stats")
        assert ev == total == len(M) * len(Q), (ev, total)


@pytest.mark.gpu
def test_search_kernels_on_a_large_random_map(plain_handle):
    rng = np.random.default_rng(31)
    N = 8192
    # frames drawn around 16 prototypes, so that ring keys spread and the bound prunes; four queries: two rotated frames, a prototype, noise
    proto = (rng.integers(0, 256, (16, NS, NR)) * (rng.random((16, NS, NR)) < rng.uniform(0.1, 0.6, (16, 1, 1)))).astype(np.int64)
    M = np.clip(proto[rng.integers(0, 16, N)] + rng.integers(-6, 7, (N, NS, NR)) * (rng.random((N, NS, NR)) < 0.5), 0, 255).astype(np.uint8)
    Q = np.stack([np.roll(M[4000], 13, axis=0), np.roll(M[8191], -1, axis=0), proto[3].astype(np.uint8), rng.integers(0, 256, (NS, NR)).astype(np.uint8)])
    want = search_np(M, Q, 8)
    plain_handle.set_option("ALEGO_RL_BUDGET", 3 * N)   # two chunks of queries
    got = plain_handle.debug_reloc_search(M, Q, 8)
    ev, total = plain_handle.debug_get("rl_stats")
    plain_handle.set_option("ALEGO_RL_BRUTE", 1)
    brute = plain_handle.debug_reloc_search(M, Q, 8)
    ev_b, _ = plain_handle.debug_get("rl_stats")
    plain_handle.set_option("ALEGO_RL_BRUTE", 0)
    plain_handle.set_option("ALEGO_RL_BUDGET", 1 << 22)
    for g, b, w, what in zip(got, brute, want, ("ids", "dists", "shifts")):
        assert np.array_equal(g, w), (what, g, w)
        assert np.array_equal(b, w), ("brute", what, b, w)
    assert got[0][0, 0] == 4000 and got[2][0, 0] == 13 and got[0][1, 0] == 8191 and got[2][1, 0] == 59 and (got[1][:2, 0] == 0).all()
    print(f"pairs evaluated: {ev} of {total} pruned path, {ev_b} brute force")
    assert total == 4 * N and ev_b == total and ev < total


def numpy_rc_params(t_map, st):
    Rm, tm = np.asarray(t_map, np.float64)[:3, :3], np.asarray(t_map, np.float64)[:3, 3]
    w, x, y, z = st[LD_Q_M2L:LD_Q_M2L + 4]
    Rc = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    R = Rm @ Rc.T
    rc = np.c_[R, tm - R @ st[LD_T_M2L:LD_T_M2L + 3]].reshape(12)
    params6 = np.r_[tm, np.arctan2(Rm[2, 1], Rm[2, 2]), np.arctan2(-Rm[2, 0], np.hypot(Rm[2, 1], Rm[2, 2])), np.arctan2(Rm[1, 0], Rm[0, 0])]
    return rc, params6


def check_against_emulation(p, lap_map, got, clouds, st, tag):
    """one slot's result against numpy (candidates) and the oracle's loop_icp (the verified candidate); returns the emulation's verdict"""
    Q, _ = desc_np(np.concatenate(clouds), MAX_RANGE, Z_OFFSET)
    ids, dists, shifts = search_np(lap_map["desc"], Q[None], got["n_cand"])
    assert np.array_equal(got["cand_id"], ids[0]) and np.array_equal(got["cand_dist"], dists[0]) and np.array_equal(got["cand_shift"], shifts[0]), (tag, got, ids, dists, shifts)
    want, g, t_map = emulate_verify(p, lap_map["frames"], lap_map["kp"], clouds, int(ids[0, 0]), int(shifts[0, 0]))
    accepted = bool(want["converged"] and want["fitness"] <= p.lc_fitness_max)
    assert_bit_equal(got["guess6"], g, f"{tag}: guess6")
    assert (got["n_source"], got["n_target"], got["converged"]) == (want["n_source"], want["n_target"], want["converged"]), (tag, got, want)
    assert abs(got["iterations"] - want["iterations"]) <= 1, (tag, got["iterations"], want["iterations"])
    assert np.abs(got["T"] - want["T"]).max() < 1e-5, (tag, got["T"], want["T"])
    assert np.abs(got["t_map"] - t_map).max() < 1e-5, (tag, got["t_map"], t_map)
    assert abs(got["fitness"] - want["fitness"]) < 1e-6 * max(1.0, want["fitness"]), (tag, got["fitness"], want["fitness"])
    assert got["status"] == (2 if accepted else 1) and got["verified"] == (0 if accepted else -1), (tag, got["status"], got["verified"])
    if accepted:
        rc, params6 = numpy_rc_params(got["t_map"], st)
        assert np.abs(got["rc"] - rc).max() < 1e-9 and np.abs(got["params6"] - params6).max() < 1e-9, (tag, got["rc"], rc, got["params6"], params6)
    return accepted


@pytest.mark.gpu
def test_lap_eight_queries_against_numpy_and_the_oracle(lap_map, eight):
    h, res = eight["h"], eight["res"]
    for i, (stream, k0, ang) in enumerate(QUERIES):
        tag = f"query {(stream, k0, ang)}"
        assert res[i]["n_cand"] == 4 and res[i]["applied"] == 0, tag
        assert check_against_emulation(h.params, lap_map, res[i], slot_clouds(h, i), h.debug_get("lm_state", slot=i), tag), tag
        assert res[i]["status"] == 2, tag
        dp, da = pose_error(res[i]["t_map"], stream, k0 + 1, ang)
        print(f"{tag}: frame {res[i]['cand_id'][0]} D {res[i]['cand_dist'][:2]} shift {res[i]['cand_shift'][0]} iterations {res[i]['iterations']} fitness {res[i]['fitness']:.4f} "
              f"error {dp:.4f} m {da:.5f} rad")
        assert dp < POS_TOL and da < ANG_TOL, (tag, dp, da)
        assert np.array_equal(h.debug_get("rl_query_desc", slot=i).reshape(NS, NR), desc_np(np.concatenate(slot_clouds(h, i)), MAX_RANGE, Z_OFFSET)[0]), tag


@pytest.mark.gpu
def test_apply_on_the_device_equals_the_host_calls(lap_map):
    n = len(QUERIES)
    a, b = loc_handle(lap_map, n), loc_handle(lap_map, n)
    for h in (a, b):
        feed_queries(h, QUERIES)
    ra = a.loc_relocalize(list(range(n)), apply=True)
    rb = b.loc_relocalize(list(range(n)), apply=False)
    for i in range(n):
        assert ra[i]["status"] == 2 and ra[i]["applied"] == 1 and rb[i]["applied"] == 0
        same_result({k: v for k, v in ra[i].items() if k != "applied"}, {k: v for k, v in rb[i].items() if k != "applied"})
        b.lm_apply_correction(rb[i]["rc"], slot=i)
        b.set_lm_params(rb[i]["params6"], slot=i)
        assert_bit_equal(a.debug_get("lm_state", slot=i), b.debug_get("lm_state", slot=i), f"slot {i}: lm_state after the placement")
        assert np.array_equal(a.debug_get("lm_info", slot=i), b.debug_get("lm_info", slot=i))
    worst = [0.0, 0.0]
    for step in range(2, 22):
        for i, (stream, k0, ang) in enumerate(QUERIES):
            pts = rotated_scan(a.params, stream, k0 + step, ang)
            fa, _, ma = a.scan_process(pts, stages=7, slot=i)
            fb, _, mb = b.scan_process(pts, stages=7, slot=i)
            assert fa == fb and fa >= 0
            assert_bit_equal(np.r_[ma["t"], ma["q"]], np.r_[mb["t"], mb["q"]], f"slot {i} step {step}: map pose")
            if a.debug_get("lm_info", slot=i)[LI_RUN]:
                s = a.loc_status(slot=i)
                assert s["optimized"] == 1 and s["window"] > 0, (i, step, s)
                w, x, y, z = ma["q"]
                T = np.eye(4)
                T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
                T[:3, 3] = ma["t"]
                dp, da = pose_error(T, stream, k0 + step, ang)
                worst = [max(worst[0], dp), max(worst[1], da)]
                assert dp < POS_TOL and da < ANG_TOL, (i, step, dp, da)
    print(f"track after the placement: worst {worst[0]:.4f} m {worst[1]:.5f} rad from ground truth")
    a.close()
    b.close()


@pytest.mark.gpu
def test_sixteen_slots_chunked_equal_single_calls(lap_map, eight):
    h = loc_handle(lap_map, 16)
    feed_queries(h, QUERIES)
    feed_queries(h, QUERIES, first_slot=8)
    whole = h.loc_relocalize(list(range(16)))
    h.set_option("ALEGO_LC_BUDGET", 1)                              # one slot per ICP chunk: sixteen chunks
    h.set_option("ALEGO_RL_BUDGET", 5 * len(lap_map["frames"]))     # five queries per search chunk: four chunks
    chunked = h.loc_relocalize(list(range(16)))
    rev = h.loc_relocalize(list(range(15, -1, -1)))
    for i in range(16):
        same_result(chunked[i], whole[i])
        same_result(rev[15 - i], whole[i])
        same_result(h.loc_relocalize([i])[0], whole[i])
        same_result(whole[i], eight["res"][i % 8])
        assert whole[i]["status"] == 2
    h.close()


@pytest.mark.gpu
def test_rejected_candidates_leave_the_slot_alone(lap_map):
    p = _params(lc_fitness_max=1e-6)
    h = loc_handle(lap_map, 2, p=p)
    feed_queries(h, QUERIES[:2])
    before = [(h.debug_get("lm_state", slot=i), h.debug_get("lm_info", slot=i)) for i in range(2)]
    res = h.loc_relocalize([0, 1], n_cand=3, verify=2, apply=True)
    for i in range(2):
        clouds = slot_clouds(h, i)
        Q, _ = desc_np(np.concatenate(clouds), MAX_RANGE, Z_OFFSET)
        ids, dists, shifts = search_np(lap_map["desc"], Q[None], 3)
        assert np.array_equal(res[i]["cand_id"], ids[0]) and np.array_equal(res[i]["cand_shift"], shifts[0])
        for v in range(2):   # both verified candidates are rejected by the emulation; the result reports the last one
            want, g, _ = emulate_verify(p, lap_map["frames"], lap_map["kp"], clouds, int(ids[0, v]), int(shifts[0, v]))
            assert not (want["converged"] and want["fitness"] <= p.lc_fitness_max), (i, v, want)
        assert_bit_equal(res[i]["guess6"], g, "the last candidate verified")
        assert abs(res[i]["fitness"] - want["fitness"]) < 1e-6 * max(1.0, want["fitness"])
        assert (res[i]["status"], res[i]["applied"], res[i]["verified"]) == (1, 0, -1), res[i]
        assert not res[i]["rc"].any() and not res[i]["params6"].any()
        assert_bit_equal(h.debug_get("lm_state", slot=i), before[i][0], f"slot {i}: lm_state")
        assert np.array_equal(h.debug_get("lm_info", slot=i), before[i][1])
    h.close()


@pytest.mark.gpu
def test_boundaries(lap_map):
    L = binding.lib()
    # before alego_loc_enable / alego_reloc_enable
    h = binding.Handle(_params())
    with pytest.raises(binding.AlegoError):
        h.reloc_enable(MAX_RANGE, Z_OFFSET)
    with pytest.raises(binding.AlegoError):
        h.loc_relocalize([0])
    h.close()
    h = loc_handle(lap_map, 3, reloc=False)
    with pytest.raises(binding.AlegoError):
        h.loc_relocalize([0])
    with pytest.raises(binding.AlegoError):
        h.debug_get("rl_query_desc")
    h.reloc_enable(MAX_RANGE, Z_OFFSET)
    with pytest.raises(binding.AlegoError):
        h.reloc_enable(MAX_RANGE, Z_OFFSET)   # a second call
    for bad in ([0, 0], [3], [-1]):
        with pytest.raises(binding.AlegoError):
            h.loc_relocalize(bad)
    with pytest.raises(binding.AlegoError):
        h.loc_relocalize([0], n_cand=9)
    with pytest.raises(binding.AlegoError):
        h.loc_relocalize([0], n_cand=2, verify=3)
    assert h.loc_relocalize([]) == []
    # a slot with no mapping frame: status 0 (slot 1 has had one scan: the odometry initialised, LaserMapping has not run)
    h.scan_process(rotated_scan(h.params, 1, 5, 1.0), stages=7, slot=1)
    feed_queries(h, QUERIES[:1], first_slot=2)
    r = h.loc_relocalize([0, 1, 2], apply=True)
    assert [x["status"] for x in r] == [0, 0, 2] and [x["n_cand"] for x in r] == [0, 0, 4] and [x["applied"] for x in r] == [0, 0, 1]
    # verify = 0: search only
    st = h.debug_get("lm_state", slot=2)
    s = h.loc_relocalize([2], n_cand=8, verify=0, apply=True)[0]
    assert (s["status"], s["verified"], s["applied"], s["n_cand"]) == (1, -1, 0, 8) and np.array_equal(s["cand_id"][:4], r[2]["cand_id"])
    assert_bit_equal(h.debug_get("lm_state", slot=2), st, "verify = 0 leaves the slot alone")
    h.close()
    # an empty map
    h = binding.Handle(_params(), n_slots=1)
    h.loc_enable([], 0.0)
    h.reloc_enable(MAX_RANGE, Z_OFFSET)
    for k in (5, 6):
        h.scan_process(_scan(k), stages=7)
    assert h.loc_relocalize([0])[0]["status"] == 0
    h.close()


@pytest.mark.gpu
def test_enabling_changes_no_existing_result(lap_map):
    """a 20-scan localisation run with and without alego_reloc_enable"""
    runs = []
    for reloc in (False, True):
        h = loc_handle(lap_map, 1, reloc=reloc)
        poses = []
        for k in range(20):
            flags, odom, mp = h.scan_process(_scan(k), stages=7)
            poses.append(np.r_[flags, odom["t"], odom["q"], mp["t"], mp["q"]])
        runs.append((np.array(poses), h.debug_get("lm_state"), h.debug_get("lm_info"), h.debug_get("lm_window")))
        h.close()
    for x, y, what in zip(runs[0], runs[1], ("poses", "lm_state", "lm_info", "lm_window")):
        assert_bit_equal(x, y, what)


@pytest.mark.gpu
def test_replay_relocalize_agrees_with_the_binding():
    n, start = 60, 31
    exe = os.path.join(ROOT, "examples", "replay")
    out = subprocess.run([exe, str(n), "--localize", "--relocalize", "--reloc-start", str(start), "--reloc-range", str(MAX_RANGE)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("reloc:")]
    assert len(line) == 1, out.stdout
    got = json.loads(line[0][len("reloc:"):])
    p = _params()
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    for k in range(n):
        h.scan_process(_scan(k), stages=7)
    frames = [h.map_get_keyframe(i) for i in range(h.map_status()[0])]
    h.close()
    h = binding.Handle(p)
    h.loc_enable([(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames], 0.0)
    h.reloc_enable(MAX_RANGE, float("nan"))
    for k in (start, start + 1):
        h.scan_process(_scan(k), stages=7)
    want = h.loc_relocalize([0], apply=True)[0]
    h.close()
    assert got["scan"] == start + 1 and got["status"] == want["status"] == 2 and got["applied"] == 1
    assert got["cand_id"] == want["cand_id"].tolist() and got["cand_dist"] == want["cand_dist"].tolist() and got["cand_shift"] == want["cand_shift"].tolist()
    assert got["iterations"] == want["iterations"] and got["fitness"] == want["fitness"]
    assert np.array_equal(np.array(got["t_map"], F32), want["t_map"].reshape(16)) and np.array_equal(np.array(got["params6"]), want["params6"])
    final = json.loads(out.stdout.splitlines()[-1])
    assert final["reloc_status"] == 2 and final["loc_max_dev"] < POS_TOL, final
