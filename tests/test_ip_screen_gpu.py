"""-m gpu: the f32 screens of ImageProjection's ground and edge tests (csrc/ip_pred.h) inside ip_fused_h / ip_fused_w and ipb_band, on constructed scans.

A scan holds one point per cell, placed at the cell's centre direction with a chosen f32 range (the range the kernels compute, sqrtf(x*x + y*y + z*z)
in f32, is reproduced here in numpy with the same expression and order, and the point is nudged until it comes out at the chosen value):
  rows G   vertical pairs whose slope lies within 1e-6 (relative) of tan(mount - thres) or tan(mount + thres) — the ground screen cannot decide them —
           alternating with pairs 1e-3 or 3e-2 off, which it decides;
  rows X   a row of constant range B (chosen so that B Kx is an f32 to 1.5e-9) in which two columns of every four hold fl(B Kx) + o ulps, o cycling
           through 0, +-1, +-2, +-40: every right-edge site between a B cell and its neighbour sits o ulps from the threshold d1 = d2 K (undecided
           at o = 0: the screen's band is a seventh of an ulp), the larger range on the left or on the right,
           across every wavefront, band and pass boundary and across the wrap column;
  rows Y   the same along the columns with Ky.
Everything else about such a scan is ordinary, so most sites are decided by the screens.  The premise — enough undecided AND decided sites of either
kind, from a numpy restatement of the screens on the oracle's own range image — is asserted on the CPU before anything runs on the device.

Compared bit for bit: the default path, the same kernels with ALEGO_IP_SCREEN=0 (every site through the fp64 block), the path of that geometry that
keeps the fp64 predicates at every site (ALEGO_IP_HALF=0, ALEGO_IP_FUSED=0 or ALEGO_IP_BAND=0), and the oracle."""
import numpy as np
import pytest

from alego_amd import binding, synth
from oracle import oracle_py as O
from util import assert_bit_equal, assert_ip_outputs_equal_oracle, assert_same_outputs as _same, ip_outputs, ip_run as _run

pytestmark = pytest.mark.gpu
F32 = np.float32
OFFS = (0, 1, 0, -1, 0, 2, 0, -2, 0, 40, 0, -40)   # ulps off the threshold; only a site ON it (less than 8e-9 relative: a seventh of an ulp) is undecided
DELTAS = (0.0, 1e-3, 2e-7, -1e-3, -2e-7, 3e-2, 5e-7, -3e-2, -5e-7, 1e-3, 9e-7, -1e-3, -9e-7, 3e-2)   # slope off the ground bound, relative: every other one within 1e-6


def _consts(p):
    """the screens' constants as ip_screen_consts computes them for the default kind of parameters used here"""
    tt = np.tan(p.seg_theta)
    out = {}
    for k, a in (("x", p.seg_alpha_x), ("y", p.seg_alpha_y)):
        K = (np.sin(a) + np.cos(a) * tt) / tt
        kh = F32(K)
        out[k] = (K, kh, F32(K - float(kh)))
        assert 2.01e-9 * np.sin(a) / tt * 4 < 8e-9   # the band of these parameters is the floor of ip_edge_band
    out["band"] = F32(8e-9 * (1 + 1e-6))
    tl, th = np.tan(np.deg2rad(p.sensor_mount_ang - p.ground_angle_thres)), np.tan(np.deg2rad(p.sensor_mount_ang + p.ground_angle_thres))
    out["g"] = (F32(np.copysign(tl * tl, tl)), F32(np.copysign(th * th, th)), F32(max(tl * tl, th * th) * (1 + 1e-6)), tl, th)
    return out


def _edge_screen_np(d1, d2, kh, kl, band):
    """ip_edge_screen on f32 arrays: (yes, und).  The fma residual of the product is exact, so fp64 arithmetic restates it."""
    d1, d2 = d1.astype(F32), d2.astype(F32)
    p = d2 * kh
    e = (d2.astype(np.float64) * float(kh) - p.astype(np.float64)).astype(F32)
    s = p - d1
    E = s + (d2.astype(np.float64) * float(kl) + e.astype(np.float64)).astype(F32)
    dec = (np.abs(E) > band * d1) & (d2 >= F32(1e-24))
    return dec & (E > 0), ~dec


def _ground_screen_np(g, fx, fy, fz):
    glo, ghi, gmax = g[:3]
    h2 = fx * fx + fy * fy
    z2 = fz * fz
    sz = np.copysign(z2, fz)
    m1, m2 = sz - glo * h2, ghi * h2 - sz
    s = z2 + gmax * h2
    tol = F32(4e-6) * s
    yes, no = (m1 > tol) & (m2 > tol), (m1 < -tol) | (m2 < -tol)
    big = s >= F32(1e-30)
    return yes & big, ~((yes | no) & big)


def _range32(xyz):
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return np.sqrt(x * x + y * y + z * z)   # f32 throughout: the kernels' expression and order (imageProjection.cpp:99)


def _ulps(v, n):
    return (np.asarray(v, F32).view(np.int32) + np.asarray(n, np.int32)).view(F32)


def _points_at(u, target):
    """f32 points along the unit directions u (f64 [.., 3]) whose f32 range is `target` exactly, found by nudging the scale and, where the roundings of
    the three squares step over the value, the direction (by 1e-4 rad: far inside the cell)"""
    best = (u * target[..., None].astype(np.float64)).astype(F32)
    hit = _range32(best) == target
    rng = np.random.default_rng(5)
    for j in range(60):
        uj = u if j == 0 else u + 1e-4 * rng.standard_normal(u.shape)
        uj = uj / np.linalg.norm(uj, axis=-1, keepdims=True)
        for k in range(-24, 25):
            if hit.all():
                return best, hit
            cand = (uj * (target.astype(np.float64) * (1.0 + k * 2.0 ** -26))[..., None]).astype(F32)
            ok = (_range32(cand) == target) & ~hit
            best[ok] = cand[ok]
            hit |= ok
    return best, hit


def _base_on_threshold(B, K):
    """per element the first f32 at or above B whose product with K lies within 1.5e-9 (relative) of an f32: fl(B K) is then a range ON the threshold"""
    B = np.asarray(B, F32)
    out = B.copy()
    done = np.zeros(B.shape, bool)
    for k in range(4000):
        c = _ulps(B, np.full(B.shape, k))
        pr = c.astype(np.float64) * K
        ok = (np.abs(pr - pr.astype(F32).astype(np.float64)) < 1.5e-9 * pr) & ~done
        out[ok] = c[ok]
        done |= ok
    assert done.all()
    return out


BOUNDARIES = (63, 127, 255, 1023)   # wavefront, band and pass boundaries of the kernels (the last column of the left side), besides the wrap column H - 1


def _rows_of(NS):
    """(G pairs' lower rows, X rows, Y rows' first row and count) of an NS-ring image"""
    if NS <= 5:
        return [0], [2], (3, 2)
    ny = 6 if NS <= 17 else 8
    return [0, 2], list(range(4, NS - ny)), (NS - ny, ny)


def near_threshold_scan(p, seed=0):
    """the constructed scan described in the module's docstring, as an (N, 4) cloud, and the per-cell f32 ranges [NS, H] it is meant to have"""
    NS, H = p.n_scan, p.horizon_scan
    c = _consts(p)
    rng = np.random.default_rng(seed)
    row, col = np.meshgrid(np.arange(NS), np.arange(H), indexing="ij")
    el = np.deg2rad(row * p.ang_res_y - p.ang_bottom)
    az = -(col + 0.5) * np.deg2rad(p.ang_res_x)
    u = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    grows, xrows, (y0, ny) = _rows_of(NS)
    tgt = np.zeros((NS, H), F32)
    off = np.array(OFFS)[(row * 5 + col * 3 + seed) % len(OFFS)]
    for b in BOUNDARIES + (H - 1,):   # next to a boundary every controlled site is on the threshold
        if b < H:
            off[:, [(b - 2) % H, b - 1, b, (b + 1) % H, (b + 2) % H]] = 0
    # rows X: the columns with (col + row) % 4 < 2 hold fl(B Kx) + o, the others B; column 0 is a K cell and the last column a B cell whatever H is,
    # so that the wrap site H - 1 | 0 is a controlled one in every row
    bk_col = (col + row) % 4 < 2
    bk_col[:, 0] = True; bk_col[:, H - 1] = False
    for r in xrows:
        B = _base_on_threshold(F32(9.0 + 0.37 * r + 0.001 * seed), c["x"][0])
        kcell = _ulps(np.full(H, F32(float(B) * c["x"][0])), off[r])
        tgt[r] = np.where(bk_col[r], kcell, B)
    # rows Y: per column a base range (neighbouring columns within 6e-4 of each other: right-edges decided), rows (r - y0) % 4 in {1, 2} at fl(B Ky) + o
    Bc = _base_on_threshold((F32(14.0 + 0.002 * seed) * (F32(1.0) + F32(1e-4) * (np.arange(H) % 7).astype(F32))).astype(F32), c["y"][0])
    for r in range(y0, y0 + ny):
        kcell = _ulps((Bc.astype(np.float64) * c["y"][0]).astype(F32), off[r])
        tgt[r] = np.where((r - y0) % 4 in (1, 2), kcell, Bc)
    pts, hit = _points_at(u, tgt)
    assert hit[xrows].mean() > 0.99 and hit[y0:y0 + ny].mean() > 0.99, "the cells of the rows X / Y cannot be given their ranges"   # (a missed cell is an ulp or two off)
    # rows G: the lower point at the cell's centre, the upper one at the range that puts the slope of their difference at tan(bound) (1 + delta)
    tl, th = c["g"][3], c["g"][4]
    for r in grows:
        cols = np.arange(H)
        r0 = 8.0 + 0.01 * (cols % 13)
        tb = np.where(cols % 2 == 0, tl, th) * (1.0 + np.array(DELTAS)[(cols // 2 + seed) % len(DELTAS)])
        e0, e1 = el[r, 0], el[r + 1, 0]
        ratio = (np.sin(e0) - tb * np.cos(e0)) / (np.sin(e1) - tb * np.cos(e1))
        r1 = np.where((ratio > 0.5) & (ratio < 2.0), r0 * ratio, r0)
        pts[r] = (u[r] * r0[:, None]).astype(F32)
        pts[r + 1] = (u[r + 1] * r1[:, None]).astype(F32)
    left = (tgt == 0)
    left[grows] = False; left[[g + 1 for g in grows]] = False
    fill = (u * (20.0 + rng.uniform(0, 5, (NS, H)))[..., None]).astype(F32)   # rows that belong to no group: an ordinary rough surface
    pts[left] = fill[left]
    cloud = np.zeros((NS * H, 4), F32)
    cloud[:, :3] = pts.reshape(-1, 3)
    cloud = cloud[rng.permutation(NS * H)]   # (the order of the points does not matter: one point per cell)
    return cloud, _range32(pts)


def assert_premise(p, o, want_rng, tag, min_edge=32, min_ground=8):
    """On the oracle's own images of the scan: the points sit in their cells with the ranges computed here, and the screens leave at least min_edge edge
    sites and min_ground ground pairs undecided and decide at least as many."""
    NS, H = p.n_scan, p.horizon_scan
    c = _consts(p)
    rimg = o.get("range_img").reshape(NS, H)
    assert_bit_equal(rimg, want_rng, f"{tag}: ranges of the constructed scan")
    act = (rimg >= 0) & (o.get("ground_img").reshape(NS, H) == 0)
    rn, an = np.roll(rimg, -1, axis=1), np.roll(act, -1, axis=1)
    sx = act & an
    _, ux = _edge_screen_np(np.maximum(rimg, rn), np.minimum(rimg, rn), c["x"][1], c["x"][2], c["band"])
    sy = act[:-1] & act[1:]
    _, uy = _edge_screen_np(np.maximum(rimg[:-1], rimg[1:]), np.minimum(rimg[:-1], rimg[1:]), c["y"][1], c["y"][2], c["band"])
    n_und, n_dec = int((ux & sx).sum() + (uy & sy).sum()), int((~ux & sx).sum() + (~uy & sy).sum())
    return n_und, n_dec, sx & ux, sy & uy


def _ground_premise(p, cloud_cells):
    c = _consts(p)
    g = min(p.ground_scan_id, p.n_scan - 1)   # pairs (row - 1, row) with row - 1 < ground_scan_id
    lo, up = cloud_cells[:g], cloud_cells[1:g + 1]
    d = up - lo
    _, und = _ground_screen_np(c["g"], d[..., 0], d[..., 1], d[..., 2])
    return int(und.sum()), int((~und).sum()), und


def _cells(p, cloud):
    """the cloud's points by cell [NS, H, 3] (the construction's directions: cell centres)"""
    NS, H = p.n_scan, p.horizon_scan
    x, y, z = cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64), cloud[:, 2].astype(np.float64)
    row = np.rint((np.rad2deg(np.arctan2(z, np.hypot(x, y))) + p.ang_bottom) / p.ang_res_y).astype(int)
    col = np.floor(np.mod(-np.arctan2(y, x), 2 * np.pi) / np.deg2rad(p.ang_res_x)).astype(int) % H
    out = np.zeros((NS, H, 3), F32)
    out[row, col] = cloud[:, :3]
    return out


def _params(geom):
    p = synth.default_params(*geom)
    if geom[0] <= 5:
        p.ground_scan_id = 1   # (a 5-ring image is all ground rows otherwise, and ground cells have no edge sites: only the pair of rows G is tested)
    return p


GEOMS = [((5, 64), "ALEGO_IP_HALF"), ((16, 64), "ALEGO_IP_HALF"), ((16, 130), "ALEGO_IP_HALF"),   # ip_fused_h: a wavefront boundary at columns 127 | 128, the wrap column
         ((16, 1800), "ALEGO_IP_FUSED"),                                                            # ip_fused_h's two passes: the pass boundary 1023 | 1024 and the sixteen-lane column
         ((17, 70), "ALEGO_IP_BAND"), ((24, 320), "ALEGO_IP_BAND")]                                  # ipb_band: one partial band; a band boundary 255 | 256, the halo column


@pytest.mark.parametrize("geom,untouched", GEOMS)
def test_near_threshold_scans_bit_for_bit(geom, untouched, monkeypatch):
    p = _params(geom)
    NS, H = geom
    o = O.Oracle(p)
    for seed in (0, 1):
        pts, want_rng = near_threshold_scan(p, seed)
        o.ip(pts)
        n_und, n_dec, ux, uy = assert_premise(p, o, want_rng, f"{geom} seed {seed}")
        g_und, g_dec, gu = _ground_premise(p, _cells(p, pts))
        print(f"{geom} seed {seed}: edge sites undecided {n_und} decided {n_dec}; ground pairs undecided {g_und} decided {g_dec}")
        assert n_und >= 32 and n_dec >= n_und, f"{geom}: {n_und} undecided / {n_dec} decided edge sites"
        assert g_und >= 8 and g_dec >= g_und, f"{geom}: {g_und} undecided / {g_dec} decided ground pairs"
        for b in [c for c in BOUNDARIES + (H - 1,) if c < H]:   # undecided right-edge sites across and on both sides of every boundary the geometry has
            assert ux[:, b].any() and (ux[:, b - 1] | ux[:, b - 2]).any() and (ux[:, (b + 1) % H] | ux[:, (b + 2) % H]).any(), f"{geom}: no undecided site at column {b}"
        c = min(1024, H - 4)   # (the first column of ip_fused_h's second pass: its ground pairs belong to the sixteen-lane column of the first)
        assert gu[:, 0:4].any() and gu[:, c:c + 4].any()
        monkeypatch.delenv("ALEGO_IP_SCREEN", raising=False); monkeypatch.delenv(untouched, raising=False)
        dflt = _run(p, pts)
        monkeypatch.setenv("ALEGO_IP_SCREEN", "0")
        _same(_run(p, pts), dflt, f"{geom} seed {seed} ALEGO_IP_SCREEN=0 vs default")
        monkeypatch.delenv("ALEGO_IP_SCREEN")
        monkeypatch.setenv(untouched, "0")
        _same(_run(p, pts), dflt, f"{geom} seed {seed} {untouched}=0 vs default")
        monkeypatch.delenv(untouched)
        assert_ip_outputs_equal_oracle(dflt, o, f"{geom} seed {seed} default vs oracle")


@pytest.mark.parametrize("geom,untouched", [((16, 130), "ALEGO_IP_HALF"), ((24, 320), "ALEGO_IP_BAND")])
def test_batch_with_some_near_threshold_slots(geom, untouched, monkeypatch):
    """One batch of 8 slots, three of them holding near-threshold scans: the fp64 blocks run in some wavefronts of the launch and not in others.  Every slot
    against a one-slot handle on the path that keeps the fp64 predicates everywhere."""
    p = synth.default_params(*geom)
    nslot = 8
    scans = [near_threshold_scan(p, 3 + s)[0] if s in (1, 4, 6) else synth.scan(p, s, stream=s) for s in range(nslot)]
    monkeypatch.delenv("ALEGO_IP_SCREEN", raising=False); monkeypatch.delenv(untouched, raising=False)
    hb = binding.Handle(p, n_slots=nslot, ring_len=1)
    for s in range(nslot):
        hb.batch_load(s, 0, scans[s])
    hb.batch_run(0, 1, stages=1)
    names = ("seg_cloud", "seg_col", "seg_range", "seg_ground", "outlier", "ring_start", "ring_end")
    got = [{n: hb.debug_get(n, slot=s).copy() for n in names} for s in range(nslot)]
    hb.close()
    monkeypatch.setenv(untouched, "0")
    for s in range(nslot):
        h1 = binding.Handle(p)
        h1.scan_process(scans[s], stages=1)
        for n in names:
            assert_bit_equal(got[s][n], h1.debug_get(n), f"{geom} slot {s} {n}")
        h1.close()


@pytest.mark.parametrize("geom", [(16, 130), (24, 320)])
def test_option_switched_on_a_live_handle(geom, monkeypatch):
    """alego_debug_set_option("ALEGO_IP_SCREEN") on a live handle: off (every site through the fp64 blocks), on again, and a handle created with the
    environment variable at 0 switched on — the same near-threshold scan gives the same bits every time, those of the oracle."""
    p = synth.default_params(*geom)
    pts, _ = near_threshold_scan(p, 2)
    o = O.Oracle(p)
    o.ip(pts)

    def outputs(h):
        return ip_outputs(h, pts)

    monkeypatch.delenv("ALEGO_IP_SCREEN", raising=False)
    h = binding.Handle(p)
    first = outputs(h)
    assert_bit_equal(first["seg"], o.get("seg_cloud"), f"{geom}: segmented cloud against the oracle")
    assert_bit_equal(first["label_image"], o.get("label_img"), f"{geom}: label image against the oracle")
    for v in (0, 1, 0):
        h.set_option("ALEGO_IP_SCREEN", v)
        _same(outputs(h), first, f"{geom} set_option(ALEGO_IP_SCREEN, {v})")
    h.close()
    monkeypatch.setenv("ALEGO_IP_SCREEN", "0")
    h = binding.Handle(p)
    _same(outputs(h), first, f"{geom} created with ALEGO_IP_SCREEN=0")
    h.set_option("ALEGO_IP_SCREEN", 1)
    _same(outputs(h), first, f"{geom} created with ALEGO_IP_SCREEN=0, switched on")
    h.close()
