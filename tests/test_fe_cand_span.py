"""fe_cand's span wavefronts (kernels_fe2.hip) on constructed segmented clouds: one wavefront takes FC_SPAN consecutive sectors of a ring, its 64-point
chunks aligned to the span and not to the sectors, the occlusion / column-jump marks of three chunks in scalar registers.

Each scene is one segmented cloud written directly — ranges, columns and ground flags per ring, ring_start / ring_end — and fed to LaserOdometry
(Handle.lo_process, Oracle.set_seg + lo()).  Two comparisons, bit for bit:

  A  against the oracle: _fe_compare's set (curvature sums, occlusion marks, labels, the three index lists, the four clouds, SC_FE_ERR == 0);
  B  between spans: what fe_cand itself writes — alego_debug_get "fe_cand_counts" and the live part of "fe_cand_lists" (the first ns and the last nf
     entries of a sector) — under ALEGO_FE_SPAN=1 (one wavefront per sector, the same template) against the default span,

and the counts against the candidates a numpy restatement finds in the oracle's curvature sums and marks.

A chunk of a span starts FF_HALO = 8 staged positions before the span's first point, so chunk boundaries fall 56 + 64 m points behind a span's start:
what moves them against a sector boundary is the length of the sectors before it, not where the ring starts in the cloud.  The rings:

  lengths   every sector of a ring L points long (ring_end - ring_start = n_sectors * L), L in 0, 1, 2 (no sector / one-point sectors, which :181 skips /
            the shortest sectors), 63, 64, 65, 127, 128, 129 (a chunk more or less) and 55, 56, 57, 119, 120, 121 (a chunk boundary one before, on and
            one after a sector boundary) — every length is the first, a middle and the last sector of its span — two rings whose lengths mix L and
            L + 1, the ring of L = 0 with its 11 points, and an empty ring (ring_end < ring_start);
  boundary  rings of 72-point sectors, one pair per feature: at every sector boundary and every chunk boundary (of the per-sector spans and of the
            default spans) b of the ring sits an occlusion pair A (marks i-5..i) with i = b - 1 or b, a pair B (marks i+1..i+5) likewise, a parallel-beam
            point, or a column jump at one of the offsets -5..+4 from b; a non-ground spike in every sector gives it picks of every class;
  full      the longest ring the sensor has (horizon_scan points), every point of every sector a candidate, sharp and flat: the two ends of a list come
            as close as a ring allows (n_sectors <= 8: sector_cap - 2 = ceil(H / n_sectors) would take a ring of more than H points);
  order     64 consecutive sharp candidates across a sector boundary — every lane of a chunk — with only flat ones behind them;
  ends      the cloud's first ring starts at k = 5 behind a pair B at k = 4, its last ring ends with a sector point at k = M - 6 before a pair A at M - 5:
            the reference marks from neither (:131).
"""
import numpy as np
import pytest

from alego_amd import synth
from oracle import oracle_py as O
from util import assert_bit_equal

F32 = np.float32
DEFAULT_SPAN = 0   # FC_SPAN of kernels_fe2.hip: the whole ring (test_default_span_is_the_one_the_scenes_assume)
H = 1440
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 55, 56, 57, 119, 120, 121)
LB = 72            # sector length of the boundary rings
FEATURES = ["A-1", "A+0", "B-1", "B+0", "C"] + [f"J{o:+d}" for o in range(-5, 5)]
CASES = [(3, 0), (4, 1), (6, 0), (6, 1), (7, 1), (8, 0)]   # n_sectors, sector_formula (4, 7, 8: a last span shorter than the others under spans of 3)


def _tdiv(a, b):   # C's division
    return abs(a) // b * (1 if a >= 0 else -1)


def sector_starts(S, E, nsec, formula):
    """first point of sectors 0 .. nsec (laserOdometry.cpp:177, LO.cpp:245); sector j is [s[j], s[j + 1] - 1]"""
    if formula == 0:
        return [_tdiv(S * (nsec - j) + E * j, nsec) for j in range(nsec + 1)]
    return [S + _tdiv(j * (E - S), nsec) for j in range(nsec + 1)]


def chunk_boundaries(starts, spans):
    """first points of the chunks 1, 2, ... of every span of `spans` sectors (0: the whole ring)"""
    nsec, out = len(starts) - 1, set()
    for span in spans:
        step = span if span > 0 else nsec
        for j0 in range(0, nsec, step):
            lo, hi = starts[j0], starts[min(j0 + step, nsec)] - 1
            out.update(range(lo + 56, hi + 1, 64))
    return out


class Ring:
    """ranges, ground flags and column steps of one ring: `span` = ring_end - ring_start, 5 padding points on either side (ring_start = first + 5,
    ring_end = last - 5, as ImageProjection publishes them); position 0 is ring_start"""

    def __init__(self, span, base=50.0, tag=""):
        self.span, self.tag, self.base = span, tag, base
        n = span + 11 if span >= 0 else 0
        self.r = np.full(n, base, F32)
        self.g = np.ones(n, np.uint8)
        self.step = np.ones(n, np.int64)    # col[i + 1] - col[i]
        self.end_adj = 0                    # added to ring_end

    def at(self, pos):
        return pos + 5

    def ok(self, pos, lo=-5, hi=5):
        return self.r.size and 0 <= pos + 5 + lo and pos + 5 + hi < self.r.size

    def occl_a(self, i):   # r[i] - r[i + 1] > occl_depth, back up in steps no predicate sees
        if self.ok(i, 0, 4):
            self.r[self.at(i) + 1:self.at(i) + 5] = self.base - np.array([0.8, 0.6, 0.4, 0.2], F32)

    def occl_b(self, i):   # r[i + 1] - r[i] > occl_depth
        if self.ok(i, -3, 1):
            self.r[self.at(i) - 3:self.at(i) + 1] = self.base - np.array([0.2, 0.4, 0.6, 0.8], F32)

    def parallel(self, i):   # both neighbours further than parallel_ratio * range (base 5: 0.1), nearer than occl_depth
        if self.ok(i, -1, 1):
            self.r[self.at(i)] = self.base * 1.06

    def jump(self, i):   # |col[i + 1] - col[i]| > suppress_col_diff
        if self.ok(i, 0, 1):
            self.step[self.at(i)] = 21

    def spike(self, i):   # a non-ground point off its neighbours' range: a sharp candidate no predicate marks
        if self.ok(i, 0, 0):
            self.r[self.at(i)] = self.base * 0.992
            self.g[self.at(i)] = 0

    def zigzag(self, a, b):   # non-ground points a .. b - 1 alternating around the base: every one a sharp candidate
        for i in range(a, b):
            if self.ok(i, 0, 0):
                self.r[self.at(i)] = self.base + (0.1 if i % 2 else -0.1)
                self.g[self.at(i)] = 0


def _busy(ring):
    """a ring with candidates of both kinds, marks and jumps all along it, at strides that share no factor with a chunk or a sector"""
    for i in range(3, ring.span, 9):
        ring.spike(i)
    for i in range(7, ring.span, 23):
        (ring.occl_a if (i // 23) % 2 else ring.occl_b)(i)
    for i in range(11, ring.span, 17):
        ring.jump(i)
    return ring


def build_scene(nsec, formula):
    """-> dict(seg = what lo_process / set_seg take, P, rings = [(Ring, S, E, sector starts)], family = {feature: [ring indices]}, full, order)"""
    rings = [_busy(Ring(nsec * L, tag=f"len{L}")) for L in LENGTHS]
    rings += [_busy(Ring(nsec * 63 + nsec // 2, tag="mix63")), _busy(Ring(nsec * 128 + (nsec + 1) // 2, tag="mix128")), Ring(-10, tag="empty")]
    family = {}
    geom = sector_starts(0, nsec * LB, nsec, formula)
    bounds = sorted(set(geom[1:nsec]) | chunk_boundaries(geom, (1, DEFAULT_SPAN)))
    for f in FEATURES:
        family[f] = []
        for parity in (0, 1):
            ring = Ring(nsec * LB, base=5.0 if f == "C" else 50.0, tag=f"{f}/{parity}")
            mine = bounds[parity::2]
            for b in mine:
                if f[0] == "A":
                    ring.occl_a(b + int(f[1:]))
                elif f[0] == "B":
                    ring.occl_b(b + int(f[1:]))
                elif f == "C":
                    ring.parallel(b)
                else:
                    ring.jump(b + int(f[1:]))
            for j in range(nsec):   # the spike of sector j: as far from every boundary as the sector allows
                cand = [p for p in range(geom[j] + 6, geom[j + 1] - 6)]
                p = max(cand, key=lambda p: min([abs(p - b) for b in bounds] + [LB]))
                assert min(abs(p - b) for b in bounds) >= 8, (f, j)
                ring.spike(p)
            family[f].append(len(rings))
            rings.append(ring)
    full = Ring(H - 11, tag="full")
    for a in range(0, full.span + 1, 48):
        full.zigzag(a + 24, a + 48)
    full_i = len(rings)
    rings.append(full)
    order = Ring(nsec * 100, tag="order")
    order.zigzag(40, 125)
    order_i = len(rings)
    rings.append(order)
    # the first ring begins the cloud behind a pair B at k = 4, the last one ends it with ring_end one further (a sector point at M - 6) before a pair A at M - 5
    first = _busy(Ring(nsec * 20, tag="first"))
    first.r[4] = first.base - F32(0.8)
    first.g[5] = 0     # (off the ground: its curvature makes it a sharp candidate)
    last = _busy(Ring(nsec * 20, tag="last"))
    last.end_adj = 1
    last.r[last.r.size - 4:] = last.base - F32(0.8)
    last.g[last.r.size - 6] = 0
    rings = [first] + rings + [last]
    family = {f: [i + 1 for i in v] for f, v in family.items()}
    full_i, order_i = full_i + 1, order_i + 1

    P = synth.default_params(len(rings), H)
    P.n_sectors, P.sector_formula = nsec, formula
    P.lo_iters_surf = P.lo_iters_corner = 0
    rng_, gnd, col, rs, re_, info = [], [], [], [], [], []
    for k, ring in enumerate(rings):
        n0 = sum(a.size for a in rng_)
        S, E = n0 + 5, n0 + 5 + ring.span + ring.end_adj
        if ring.span < 0:   # no point: what ImageProjection leaves for a ring without one
            S, E = n0 + 4, n0 - 6
        rs.append(S); re_.append(E)
        rng_.append(ring.r); gnd.append(ring.g)
        col.append(np.concatenate([[0], np.cumsum(ring.step[:-1])]).astype(np.int32) if ring.r.size else np.zeros(0, np.int32))
        info.append((ring, S, E, sector_starts(S, E, nsec, formula)))
    r, g, c = np.concatenate(rng_), np.concatenate(gnd), np.concatenate(col)
    assert c.max() < 32768 and max(a.size for a in rng_) <= H and r.size <= len(rings) * H
    ring_of = np.concatenate([np.full(a.size, k, np.int32) for k, a in enumerate(rng_)])
    pts = np.stack([r, F32(0.05) * np.arange(r.size, dtype=F32) % F32(60), F32(0.5) * ring_of.astype(F32), ring_of.astype(F32) + c.astype(F32) / F32(10000)], 1).astype(F32)
    seg = dict(seg=pts, ground=g, col=c, range=r, ring_start=np.asarray(rs, np.int32), ring_end=np.asarray(re_, np.int32), orientation=np.zeros(3, F32))
    return dict(seg=seg, P=P, rings=info, family=family, full=full_i, order=order_i, bounds=bounds, nsec=nsec)


def expected_counts(sc, curv_d, picked):
    """[ring][sector][2]: the sharp / flat candidates of every sector with two points or more (:181), from the oracle's curvature sums and marks"""
    P, seg = sc["P"], sc["seg"]
    curv = np.abs(curv_d).astype(np.float64) ** 2
    free = picked == 0
    sharp = free & (seg["ground"] == 0) & (curv > P.edge_thres)
    flat = free & (seg["ground"] != 0) & (curv < P.surf_thres)
    out = np.zeros((len(sc["rings"]), sc["nsec"], 2), np.int32)
    for k, (_, S, E, st) in enumerate(sc["rings"]):
        for j in range(sc["nsec"]):
            sp, ep = st[j], st[j + 1] - 1
            if sp < ep:
                out[k, j] = sharp[sp:ep + 1].sum(), flat[sp:ep + 1].sum()
    return out, sharp, flat


def run_oracle(sc):
    o = O.Oracle(sc["P"])
    o.set_seg(sc["seg"])
    o.lo()
    return o


_SCENES = {}


def scene(nsec, formula):
    """the scene and what the oracle makes of it, computed once per case"""
    key = (nsec, formula)
    if key not in _SCENES:
        sc = build_scene(nsec, formula)
        o = run_oracle(sc)
        sc["curv_d"], sc["picked"] = o.get("curv_d"), o.get("picked_occl")
        sc["idx"] = {n: o.get(n + "_idx") for n in ("sharp", "less_sharp", "flat")}
        sc["want"], sc["cs"], sc["cf"] = expected_counts(sc, sc["curv_d"], sc["picked"])
        o.close()
        _SCENES[key] = sc
    return _SCENES[key]


@pytest.mark.parametrize("nsec,formula", CASES)
def test_scene_holds_what_it_was_built_for(nsec, formula):
    """from the oracle's outputs alone: the sector lengths, the marks on both sides of every boundary, picks of every class in every boundary sector,
    the cloud's ends, the full lists and the chunk of sharp candidates"""
    sc = scene(nsec, formula)
    M, picked, cs, cf, want = sc["seg"]["range"].size, sc["picked"], sc["cs"], sc["cf"], sc["want"]
    by_tag = {ring.tag: (ring, S, E, st) for ring, S, E, st in sc["rings"]}
    for L in LENGTHS:
        st = by_tag[f"len{L}"][3]
        assert [st[j + 1] - st[j] for j in range(nsec)] == [L] * nsec, (L, st)
    assert by_tag["len0"][0].r.size == 11 and by_tag["empty"][2] < by_tag["empty"][1]
    assert want[[k for k, x in enumerate(sc["rings"]) if x[0].tag in ("len0", "len1", "empty")]].sum() == 0
    assert want[[k for k, x in enumerate(sc["rings"]) if x[0].tag == "len2"]].sum() > 0
    for b in sc["bounds"]:   # a mark within five points on either side of every boundary, from the occlusion pairs and the parallel point
        left = right = False
        for f in ("A-1", "A+0", "B-1", "B+0", "C"):
            for k in sc["family"][f]:
                S = sc["rings"][k][1]
                left |= bool(picked[S + b - 5:S + b].any())
                right |= bool(picked[S + b:S + b + 5].any())
        assert left and right, f"boundary {b}: marks left {left} right {right}"
    jumps = np.abs(np.diff(sc["seg"]["col"])) > sc["P"].suppress_col_diff
    for f in FEATURES[5:]:   # the column jump sits where it was put, at every boundary of its pair of rings
        for parity, k in enumerate(sc["family"][f]):
            S = sc["rings"][k][1]
            assert all(jumps[S + b + int(f[1:])] for b in sc["bounds"][parity::2]), f
    for f in FEATURES:       # picks of every class, and candidates of both kinds, in every sector of the boundary rings
        for k in sc["family"][f]:
            st = sc["rings"][k][3]
            for j in range(nsec):
                for name in ("sharp", "less_sharp", "flat"):
                    ix = sc["idx"][name]
                    assert ((ix >= st[j]) & (ix < st[j + 1])).any(), f"ring {sc['rings'][k][0].tag} sector {j}: no {name} pick"
                assert want[k, j, 0] > 0 and want[k, j, 1] > 0
    assert sc["rings"][0][1] == 5 and sc["rings"][-1][3][nsec] - 1 == M - 6, "the first sector point is k = 5, the last one k = M - 6"
    assert cs[5] and cs[M - 6], "candidates at both ends of the cloud"
    assert picked[5:10].sum() == 0 and picked[M - 6] == 0, "the reference marks from neither k = 4 nor k = M - 5"
    st = sc["rings"][sc["full"]][3]
    lens = [st[j + 1] - st[j] for j in range(nsec)]
    j = int(np.argmax(lens))
    assert want[sc["full"], j].sum() == lens[j] == -(-(H - 11) // nsec) and want[sc["full"], j].min() > 0, (lens, want[sc["full"]])
    S = sc["rings"][sc["order"]][1]
    assert cs[S + 40:S + 125].all() and not cs[S + 125:S + 200].any() and cf[S + 131:S + 195].all()


def _live(counts, lists, cap):
    """the live entries of every sector's list: (ring, sector, first ns entries, last nf entries)"""
    nr, nsec = counts.shape[:2]
    L = lists.reshape(nr, nsec, cap, 2)
    return [(k, j, L[k, j, :counts[k, j, 0]].copy(), L[k, j, cap - counts[k, j, 1]:].copy()) for k in range(nr) for j in range(nsec)]


def _fe_cand_outputs(h, nr, nsec):
    span, cap = h.debug_get("fe_cand_span")
    counts = h.debug_get("fe_cand_counts").reshape(nr, nsec, 2)
    return int(span), counts, _live(counts, h.debug_get("fe_cand_lists"), int(cap))


def _assert_same_lists(got, want, tag):
    span_g, counts_g, live_g = got
    span_w, counts_w, live_w = want
    assert span_w == 1 and span_g == DEFAULT_SPAN, (span_g, span_w)
    assert_bit_equal(counts_g, counts_w, f"{tag}: fe_cand_counts, default span against one sector per wavefront")
    for (k, j, s_g, f_g), (_, _, s_w, f_w) in zip(live_g, live_w):
        assert_bit_equal(s_g, s_w, f"{tag}: ring {k} sector {j} sharp candidates")
        assert_bit_equal(f_g, f_w, f"{tag}: ring {k} sector {j} flat candidates")


@pytest.mark.gpu
def test_default_span_is_the_one_the_scenes_assume():
    from alego_amd import binding
    h = binding.Handle(synth.default_params(16, 1800))
    assert h.debug_get("fe_cand_span")[0] == DEFAULT_SPAN
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cand", [0, 8], ids=["default", "cand8"])
@pytest.mark.parametrize("nsec,formula", CASES)
def test_span_scene_device(nsec, formula, cand, monkeypatch):
    """comparisons A and B on the constructed scene; cand8: ALEGO_FE_CAND=8, so that the span lists feed ff_pick_mem too"""
    from alego_amd import binding
    from test_gpu_parity import _fe_compare
    sc = scene(nsec, formula)
    if cand:
        monkeypatch.setenv("ALEGO_FE_CAND", str(cand))
    nr = len(sc["rings"])
    out = {}
    for span in ("1", None):
        if span:
            monkeypatch.setenv("ALEGO_FE_SPAN", span)
        else:
            monkeypatch.delenv("ALEGO_FE_SPAN", raising=False)
        h, o = binding.Handle(sc["P"]), run_oracle(sc)
        flags, feat, odom = h.lo_process(sc["seg"])
        _fe_compare(h, o, feat, f"{nsec} sectors, formula {formula}, span {span or 'default'}")
        out[span] = _fe_cand_outputs(h, nr, nsec)
        assert_bit_equal(out[span][1], sc["want"], f"span {span or 'default'}: fe_cand_counts against the candidates in the oracle's curvature sums and marks")
        h.close(); o.close()
    _assert_same_lists(out[None], out["1"], f"{nsec} sectors, formula {formula}")


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(16, 1800), (16, 4000), (64, 2048)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_span_synth_geometries(geom, monkeypatch):
    """comparison B on three scans of the synthetic stream at the workload's geometries"""
    from alego_amd import binding
    p = synth.default_params(*geom)
    monkeypatch.setenv("ALEGO_FE_SPAN", "1")
    h1 = binding.Handle(p)
    monkeypatch.delenv("ALEGO_FE_SPAN")
    h = binding.Handle(p)
    for k in range(3):
        pts = synth.scan(p, k)
        h1.scan_process(pts, stages=7, want_outputs=True)
        h.scan_process(pts, stages=7, want_outputs=True)
        got, want = _fe_cand_outputs(h, p.n_scan, p.n_sectors), _fe_cand_outputs(h1, p.n_scan, p.n_sectors)
        assert want[1].sum() > 0
        _assert_same_lists(got, want, f"{geom} scan {k}")
    h.close(); h1.close()
