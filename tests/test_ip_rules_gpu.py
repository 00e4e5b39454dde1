"""-m gpu: the output rules of ImageProjection (csrc/ip_rules.h) through every kernel path, on scans built to sit on the rules' thresholds.

A scan holds at most one point per cell, at the cell's centre direction.  Rows 0 and 1 are a flat floor (ground wherever ground_scan_id lets the pair be
tested); above them, in bands of three rows, lie blobs of constant range with empty cells all around, so that each is one segment of exactly
  4 cells (2 + 2), 5 cells over 2 rows (3 + 2) or over 3 (2 + 2 + 1), 29 cells over 2 rows (15 + 14) or over 3 (10 + 10 + 9), 30 cells (15 + 15):
with the default thresholds (30 / 5 cells / 3 rings) the 5- and 29-cell ones over 3 rows and the 30-cell one are feasible, the others are not.
A blob starts at column 0 (inside columns 0 - 4), at column 20 (a multiple of 5), at column 36 (none), ends at column H - 1 (inside H - 5 .. H - 1 when it
is narrow) or straddles the wrap column; shapes rotate through these places from scan to scan and band to band.  The premise — every blob is the segment
it is meant to be, none of its cells is ground, the floor is ground when the pair is tested — is asserted on the oracle's images before anything runs on
the device, and so is that every place saw all four sizes.

Crossed with ground_scan_id in -1, 0, NS - 2, NS - 1, NS + 3.  Compared bit for bit, per scan: every kernel path the geometry has against the oracle and
against the geometry's first path — segmented cloud, its ground / column / range arrays, outliers, ring indices, the three totals, label image.
16 x 2050 stands for 16 x 4000: it is the narrowest 16-ring image that ip_fused_h refuses (N > 32768) and ip_fused_w takes."""
import numpy as np
import pytest

from alego_amd import binding, synth
from oracle import oracle_py as O
from util import IP_ORACLE_NAMES, assert_bit_equal, assert_ip_outputs_equal_oracle, assert_same_outputs, ip_outputs

pytestmark = pytest.mark.gpu
F32 = np.float32
SC_M, SC_NOUT, SC_NFEAS = 3, 4, 5   # csrc/fe_store.h

SHAPES = [(2, 2), (3, 2), (2, 2, 1), (15, 14), (10, 10, 9), (15, 15)]   # cells per row, bottom-up, left-aligned
FEASIBLE = [False, False, True, False, True, True]

# geometry -> the switch sets of its paths; the first is the default path
PATHS = {
    (5, 64): [{}, {"ALEGO_IP_HALF": "0"}],                                                   # ip_fused_h; ip_fused
    (16, 130): [{}, {"ALEGO_IP_HALF": "0"}, {"ALEGO_IP_FUSED": "0"},                         # ip_fused_h; ip_fused; cc_lds16 with its compaction;
                {"ALEGO_IP_FUSED": "0", "ALEGO_CC_FUSED": "0"}],                             # cc_lds16 + ip_rowcount + ip_compact
    (16, 2050): [{}, {"ALEGO_IP_FUSED": "0"}],                                               # ip_fused_w; cc_lds16 with its compaction
    (17, 70): [{}, {"ALEGO_IP_BAND": "0"}],                                                  # banded; cc_lds + cc_stats + ip_rowcount + ip_compact
    (24, 320): [{}, {"ALEGO_IP_BAND": "0"}],
}
SWITCHES = ("ALEGO_IP_HALF", "ALEGO_IP_FUSED", "ALEGO_CC_FUSED", "ALEGO_IP_BAND")


def _bands(NS):
    return [r for r in range(2, NS - 2, 4)]   # first row of every band of three rows, an empty row between two bands


def _n_scans(NS):
    return 18 if len(_bands(NS)) == 1 else 9


def blob_layout(NS, H, s):
    """the blobs of scan s: (place, shape index, first row, first column); columns run on across the wrap.  A band holds one blob at an end of the image
    (at column 0, up to column H - 1, or across the wrap: two of them would touch through the wrap) and up to two in the middle."""
    out = []
    for b, row0 in enumerate(_bands(NS)):
        kind, turn = (s + b) % 3, (s + b) // 3 + 2 * b

        def shape(z):
            return (z + turn) % len(SHAPES)

        w = SHAPES[shape(0)][0]
        first = (0, H - w, H - (w + 1) // 2)[kind]
        out.append((("col0", "end", "wrap")[kind], shape(0), row0, first))
        out.append(("mult5", shape(1), row0, 20))
        if 36 + SHAPES[shape(2)][0] < (first if kind else H - 8):   # (an empty column between two blobs, also through the wrap)
            out.append(("nonmult", shape(2), row0, 36))
    return out


def blob_cells(H, blob):
    _, k, row0, col0 = blob
    return [(row0 + dr, (col0 + dc) % H) for dr, n in enumerate(SHAPES[k]) for dc in range(n)]


def rules_scan(p, s):
    """scan s as an (n, 4) cloud, and its blobs"""
    NS, H = p.n_scan, p.horizon_scan
    rng = np.random.default_rng(100 + s)
    row, col = np.meshgrid(np.arange(NS), np.arange(H), indexing="ij")
    el = np.deg2rad(row * p.ang_res_y - p.ang_bottom)
    az = -(col + 0.5) * np.deg2rad(p.ang_res_x)
    u = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    r = np.zeros((NS, H))
    assert el[1, 0] < np.deg2rad(-5.0)
    r[:2] = 2.0 / np.sin(-el[:2])   # the floor, 2 m below the sensor
    blobs = blob_layout(NS, H, s)
    for i, blob in enumerate(blobs):
        for cell in blob_cells(H, blob):
            r[cell] = 3.0 + 0.2 * i   # (nearer than the floor under it: the step from the floor up to a blob is steeper than any ground slope)
    # two lone cells on multiples of 5, infeasible segments of one cell: in the bottom row (a hole in the floor around it), an outlier only below
    # ground_scan_id = 0, and in the top row where the blobs leave room, an outlier only up to ground_scan_id = NS - 2
    r[:2, 9:12] = 0.0
    r[0, 10] = 7.0
    lone = [(0, 10)]
    for c in range(H - H % 5 - 5, 0, -5):
        if not r[NS - 2:, c - 1:c + 2].any():
            r[NS - 1, c] = 7.0
            lone.append((NS - 1, c))
            break
    keep = r > 0
    cloud = np.zeros((int(keep.sum()), 4), F32)
    cloud[:, :3] = (u[keep] * r[keep][:, None]).astype(F32)
    return cloud[rng.permutation(cloud.shape[0])], blobs, lone


def assert_premise(p, o, blobs, lone, tag):
    NS, H = p.n_scan, p.horizon_scan
    lab, gnd = o.get("label_img").reshape(NS, H), o.get("ground_img").reshape(NS, H)
    floor = o.get("range_img").reshape(NS, H)[:2] > 0
    floor[0, 10] = False
    assert floor[0].sum() == H - 3 and (floor[0] == floor[1]).all(), f"{tag}: the floor is not where it was put"
    if p.ground_scan_id >= 1:
        assert gnd[:2][floor].all(), f"{tag}: the floor is not ground"
    else:
        assert not gnd.any(), f"{tag}: ground although no pair is tested"
    for cell in lone:
        assert lab[cell] == 999999 and not gnd[cell], f"{tag}: the lone cell {cell} is no infeasible segment"
    n_out = sum(1 for row, _ in lone if row > p.ground_scan_id)
    for blob in blobs:
        if not FEASIBLE[blob[1]]:
            n_out += sum(1 for row, col in blob_cells(H, blob) if col % 5 == 0 and row > p.ground_scan_id)
    assert o.get("outlier").shape[0] == n_out, f"{tag}: {o.get('outlier').shape[0]} outliers, {n_out} by the rule"
    for blob in blobs:
        cells = blob_cells(H, blob)
        rr, cc = np.array(cells).T
        size = sum(SHAPES[blob[1]])
        assert len(cells) == size and not gnd[rr, cc].any(), f"{tag}: {blob}: ground cells in the blob"
        ls = lab[rr, cc]
        if FEASIBLE[blob[1]]:
            assert ls[0] > 0 and ls[0] < 999999 and (ls == ls[0]).all() and int((lab == ls[0]).sum()) == size, f"{tag}: {blob} is not one feasible segment of {size} cells: {ls}"
        else:
            assert (ls == 999999).all(), f"{tag}: {blob} is not an infeasible segment: {ls}"


def test_every_place_sees_every_size():
    for NS, H in PATHS:
        seen = {}
        assert any(len(rules_scan(synth.default_params(NS, H), s)[2]) == 2 for s in range(_n_scans(NS))), f"{NS}x{H}: no scan has room for the lone cell of the top row"
        for s in range(_n_scans(NS)):
            for place, k, _, _ in blob_layout(NS, H, s):
                seen.setdefault(place, set()).add(k)
        for place in ("col0", "mult5", "nonmult", "end", "wrap"):
            sizes = {sum(SHAPES[k]) for k in seen.get(place, ())}
            assert sizes == {4, 5, 29, 30}, f"{NS}x{H}: {place} saw the sizes {sorted(sizes)}"
        assert set().union(*seen.values()) == set(range(len(SHAPES))), f"{NS}x{H}: shapes {seen}"


def _totals(o):
    lab = o.get("label_img")
    return np.array([o.get("seg_cloud").shape[0], o.get("outlier").shape[0], np.unique(lab[(lab > 0) & (lab < 999999)]).size], np.int32)


class _Kept:
    """the oracle's arrays of one scan, kept while it goes on to the next: every path is compared scan by scan against them"""
    NAMES = ("range_img", "ground_img", "label_img") + tuple(n for _, n in IP_ORACLE_NAMES)

    def __init__(self, o):
        self.d = {n: o.get(n).copy() for n in self.NAMES}
        self.totals = _totals(o)

    def get(self, n):
        return self.d[n]


@pytest.mark.parametrize("gsi_of", ["-1", "0", "NS-2", "NS-1", "NS+3"])
@pytest.mark.parametrize("geom", list(PATHS))
def test_threshold_segments_on_every_path(geom, gsi_of, monkeypatch):
    NS, H = geom
    p = synth.default_params(*geom)
    p.ground_scan_id = {"-1": -1, "0": 0, "NS-2": NS - 2, "NS-1": NS - 1, "NS+3": NS + 3}[gsi_of]
    o = O.Oracle(p)
    scans, want = [], []
    for s in range(_n_scans(NS)):
        pts, blobs, lone = rules_scan(p, s)
        o.ip(pts)
        assert_premise(p, o, blobs, lone, f"{geom} gsi {p.ground_scan_id} scan {s}")
        scans.append(pts)
        want.append(_Kept(o))
    first = None
    for sw in PATHS[geom]:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        h = binding.Handle(p)   # one handle per path, the scans one after the other
        got = []
        for s, pts in enumerate(scans):
            tag = f"{geom} gsi {p.ground_scan_id} scan {s} {sw or 'default'}"
            out = ip_outputs(h, pts)
            assert_ip_outputs_equal_oracle(out, want[s], f"{tag} vs oracle")
            out["totals"] = np.asarray(h.debug_get("scal"), np.int32)[[SC_M, SC_NOUT, SC_NFEAS]].copy()
            assert_bit_equal(out["totals"], want[s].totals, f"{tag} vs oracle: kept cells, outliers, feasible segments")
            got.append(out)
        h.close()
        if first is None:
            first = got
        else:
            for s in range(len(scans)):
                assert_same_outputs(got[s], first[s], f"{geom} gsi {p.ground_scan_id} scan {s} {sw} vs default")
