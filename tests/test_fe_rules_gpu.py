"""Every pick path of feature extraction against the oracle, bit for bit, at the smallest shapes at which a rule of csrc/fe_rules.h can go wrong:
one constructed segmented cloud of 16 rings by 72 columns, one scan, one slot.

Paths: the default (fe_cand + fe_pickc + fe_ring_out), ALEGO_FE_SPAN=1 (one fe_cand wavefront per sector), ALEGO_FE_CAND=8 (ff_pick_mem), ALEGO_FE_FUSED=0
(fe_curv + fe_pick4 + fe_voxel + fe_collect), that with ALEGO_FE_PICK1=1 (fe_pick), and the last two again with sort_mode = 2 (std::sort's tie order).
Parameter sets, each within what alego_create accepts: n_sectors 1, 6, 7 and 24 with both sector formulas; suppress_radius 0, 1 and 5 with suppress_col_diff = 2,
so that the scan's dropped columns (column steps of 3) cut the reach; n_sharp = 0, n_less_sharp = n_sharp, n_flat = 1; occl_f32 = 1 (0 is every other set).
Compared as test_gpu_parity._fe_compare does: curvature sums, occlusion marks, labels, the three index lists, the four clouds, SC_FE_ERR == 0.

The rings (spans = ring_end - ring_start): 61 (the longest a 72-column ring allows), 60, 48, 42, 37, 30, 24, 19, 13, 7 and 6 (one-point sectors under 7 / 6
sectors and more, which :181 skips), 1, 0, a ring without a point (ring_end < ring_start), and two rings of constant range whose flat candidates all tie at
curvature 0 — one of them with a run of alternating non-ground points, whose sharp candidates tie as well.
test_scenes_hold_what_the_rules_need asserts on the CPU, from the oracle's own inputs and outputs over all cases, that each of these occurs: a skipped
one-point sector, an empty ring, a suppression cut short by a column jump, two candidates of equal curvature in one sector, a sector whose flat loop stops
at n_flat.

test_no_sharp_features_through_laser_odometry: n_sharp = 0 once more with LaserOdometry iterating, on two scans at 16 x 1800."""
import numpy as np
import pytest

from alego_amd import synth
from oracle import oracle_py as O
from test_fe_cand_span import Ring, sector_starts

F32 = np.float32
NS, H = 16, 72
SPANS = (61, 60, 48, 42, 37, 30, 24, 19, 13, 7, 6, 1, 0, -10)

PARAMS = [(f"nsec{n}-f{f}", dict(n_sectors=n, sector_formula=f)) for n in (1, 6, 7, 24) for f in (0, 1)]
PARAMS += [(f"radius{r}", dict(suppress_radius=r, suppress_col_diff=2)) for r in (0, 1, 5)]
PARAMS += [("nsharp0", dict(n_sharp=0)), ("nls_eq_ns", dict(n_sharp=2, n_less_sharp=2)), ("nflat1", dict(n_flat=1)), ("occl_f32", dict(occl_f32=1))]
PATHS = [("default", {}, 0), ("span1", {"ALEGO_FE_SPAN": "1"}, 0), ("cand8", {"ALEGO_FE_CAND": "8"}, 0), ("unfused", {"ALEGO_FE_FUSED": "0"}, 0),
         ("pick1", {"ALEGO_FE_FUSED": "0", "ALEGO_FE_PICK1": "1"}, 0), ("unfused_sort2", {"ALEGO_FE_FUSED": "0"}, 2),
         ("pick1_sort2", {"ALEGO_FE_FUSED": "0", "ALEGO_FE_PICK1": "1"}, 2)]


def _features(ring, k):
    """candidates of both kinds, marks of all three kinds, column jumps (steps of 21) and dropped columns (steps of 3) along a ring, at strides that share
    no factor with a sector"""
    for i in range(2 + k % 3, ring.span, 7):
        ring.spike(i)
    for i in range(5 + k % 4, ring.span, 19):
        (ring.occl_a if (i // 19 + k) % 2 else ring.occl_b)(i)
    for i in range(9 + k % 5, ring.span, 13):
        ring.jump(i)
    for i in range(1 + k % 2, ring.span, 5):
        if ring.ok(i, 0, 1) and ring.step[ring.at(i)] == 1:
            ring.step[ring.at(i)] = 3
    return ring


def _scene():
    rings = [_features(Ring(s, base=5.0 if k == 3 else 50.0, tag=f"span{s}"), k) for k, s in enumerate(SPANS)]
    rings[3].parallel(20)                       # (base 5: both neighbours further than parallel_ratio * range, nearer than occl_depth)
    flat = Ring(55, tag="ties")                 # constant range: every curvature sum is 0
    for i in range(4, flat.span, 11):
        flat.step[flat.at(i)] = 3
    both = Ring(50, tag="ties2")
    both.zigzag(10, 30)                         # alternating non-ground points: equal |curvature sum| in the middle of the run
    for i in range(3, both.span, 6):
        both.step[both.at(i)] = 3
    rings += [flat, both]
    assert len(rings) == NS
    rng_, gnd, col, rs, re_ = [], [], [], [], []
    for ring in rings:
        n0 = sum(a.size for a in rng_)
        S, E = (n0 + 5, n0 + 5 + ring.span) if ring.span >= 0 else (n0 + 4, n0 - 6)   # (no point: what ImageProjection leaves for such a ring)
        rs.append(S); re_.append(E)
        rng_.append(ring.r); gnd.append(ring.g)
        col.append(np.concatenate([[0], np.cumsum(ring.step[:-1])]).astype(np.int32) if ring.r.size else np.zeros(0, np.int32))
    r, g, c = np.concatenate(rng_), np.concatenate(gnd), np.concatenate(col)
    assert max(a.size for a in rng_) <= H and c.max() < 32768
    ring_of = np.concatenate([np.full(a.size, k, np.int32) for k, a in enumerate(rng_)])
    pts = np.stack([r, F32(0.05) * np.arange(r.size, dtype=F32) % F32(60), F32(0.5) * ring_of.astype(F32), ring_of.astype(F32) + c.astype(F32) / F32(10000)], 1).astype(F32)
    return dict(seg=pts, ground=g, col=c, range=r, ring_start=np.asarray(rs, np.int32), ring_end=np.asarray(re_, np.int32), orientation=np.zeros(3, F32))


SEG = _scene()
_ORACLE = {}


def _params(mods, sort_mode):
    P = synth.default_params(NS, H)
    P.lo_iters_surf = P.lo_iters_corner = 0
    for k, v in mods.items():
        setattr(P, k, v)
    P.sort_mode = sort_mode
    return P


def _oracle_outputs(name, sort_mode):
    """what the oracle makes of the scene under a parameter set, computed once and left unchanged"""
    key = (name, sort_mode)
    if key not in _ORACLE:
        P = _params(dict(PARAMS)[name], sort_mode)
        o = O.Oracle(P)
        o.set_seg(SEG)
        o.lo()
        out = {n: o.get(n).copy() for n in ("seg_cloud", "curv_d", "picked_occl", "point_label", "sharp_idx", "less_sharp_idx", "flat_idx", "sharp", "less_sharp", "flat", "less_flat")}
        o.close()
        _ORACLE[key] = out
    return _ORACLE[key]


class _Frozen:
    """the cached outputs behind the oracle's get(), for _fe_compare"""

    def __init__(self, out):
        self.out = out

    def get(self, name):
        return self.out[name]


def _counts(name, sort_mode):
    """from the oracle's inputs and outputs: [skipped one-point sectors, empty rings, suppressions cut short by a column jump, sectors with two candidates
    of equal curvature, sectors whose flat loop stops at n_flat]"""
    P, out = _params(dict(PARAMS)[name], sort_mode), _oracle_outputs(name, sort_mode)
    curv = np.abs(out["curv_d"]).astype(np.float64) ** 2
    free = out["picked_occl"] == 0
    sharp_c = free & (SEG["ground"] == 0) & (curv > P.edge_thres)
    flat_c = free & (SEG["ground"] != 0) & (curv < P.surf_thres)
    jump = np.abs(np.diff(SEG["col"])) > P.suppress_col_diff            # between k and k + 1
    n = np.zeros(5, np.int64)
    for S, E in zip(SEG["ring_start"], SEG["ring_end"]):
        if E < S:
            n[1] += 1
            continue
        st = sector_starts(int(S), int(E), P.n_sectors, P.sector_formula)
        for j in range(P.n_sectors):
            sp, ep = st[j], st[j + 1] - 1
            n[0] += sp == ep
            if sp >= ep:
                continue
            for cand in (sharp_c, flat_c):
                keys = np.abs(out["curv_d"][sp:ep + 1][cand[sp:ep + 1]])
                n[3] += np.unique(keys).size < keys.size
            flats = [c for c in out["flat_idx"] if sp <= c <= ep]
            n[4] += len(flats) == P.n_flat
            spreading = [c for c in out["less_sharp_idx"] if sp <= c <= ep] + flats[:P.n_flat - 1]   # (the n_flat-th flat pick does not spread)
            for c in spreading:
                n[2] += bool(jump[c:c + P.suppress_radius].any() or jump[c - P.suppress_radius:c].any())
    return n


def test_scenes_hold_what_the_rules_need():
    total = sum(_counts(name, sm) for name, _ in PARAMS for sm in (0, 2))
    print("one-point sectors, empty rings, cut suppressions, tied sectors, full flat sectors:", total)
    assert (total >= 1).all(), total
    for name in ("radius1", "radius5"):
        assert _counts(name, 0)[2] >= 1, f"{name}: no suppression cut short by a dropped column"
    assert _counts("nsec7-f0", 0)[0] >= 1 and _counts("nsec24-f1", 0)[0] >= 1 and _counts("nflat1", 0)[4] >= 1
    assert _counts("nsec1-f0", 2)[3] >= 1, "sort_mode 2 has ties to order"
    assert len(_oracle_outputs("nsharp0", 0)["sharp_idx"]) == 0 and len(_oracle_outputs("nsharp0", 0)["less_sharp_idx"]) > 0
    o = _oracle_outputs("nls_eq_ns", 0)
    assert len(o["sharp_idx"]) > 0 and np.array_equal(o["sharp_idx"], o["less_sharp_idx"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", [p[0] for p in PATHS])
@pytest.mark.parametrize("name", [p[0] for p in PARAMS])
def test_pick_paths_equal_the_oracle(name, path, monkeypatch):
    from alego_amd import binding
    from test_gpu_parity import _fe_compare
    _, env, sort_mode = next(p for p in PATHS if p[0] == path)
    for k in ("ALEGO_FE_SPAN", "ALEGO_FE_CAND", "ALEGO_FE_FUSED", "ALEGO_FE_PICK1"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = binding.Handle(_params(dict(PARAMS)[name], sort_mode))
    flags, feat, odom = h.lo_process(SEG)
    _fe_compare(h, _Frozen(_oracle_outputs(name, sort_mode)), feat, f"{name} {path}")
    h.close()


@pytest.mark.gpu
def test_no_sharp_features_through_laser_odometry():
    """n_sharp = 0 with LaserOdometry's iterations on, two scans of the synthetic stream at 16 x 1800: the sharp cloud is empty (laserOdometry.cpp:196), so the
    corner loop (:427) has no query and the second solve runs on the surf rows alone.  Features bit for bit, no corner correspondence on either side, surf
    correspondences equal, the pose parameters within 1e-7 (test_gpu_parity's bound for a teacher-forced scan)."""
    from alego_amd import binding
    from test_gpu_parity import _fe_compare, _ip_compare
    p = synth.default_params(16, 1800)
    p.n_sharp = 0
    h, o = binding.Handle(p), O.Oracle(p)
    for k in range(2):
        seg = _ip_compare(h, o, synth.scan(p, k), f"n_sharp 0 scan {k}")
        h.set_lo_params(o.get("lo_params"))
        ok = o.lo()
        flags, feat, odom = h.lo_process(seg)
        _fe_compare(h, o, feat, f"n_sharp 0 scan {k}")
        assert feat["sharp"].shape[0] == 0 and feat["less_sharp"].shape[0] > 0
        if k == 0:
            continue
        assert ok and odom["valid"]
        gc = h.debug_get("lo_surf_corr").reshape(-1, 4)
        np.testing.assert_array_equal(gc[gc[:, 1] >= 0], o.get("lo_surf_corr").reshape(-1, 4))
        assert o.get("lo_corner_corr").size == 0
        cc = h.debug_get("lo_corner_corr").reshape(-1, 4)
        assert cc[cc[:, 1] >= 0].shape[0] == 0
        np.testing.assert_allclose(odom["params"], o.get("lo_params"), rtol=0, atol=1e-7, err_msg="params_ after the corner solve without corner rows")
    h.close(); o.close()
