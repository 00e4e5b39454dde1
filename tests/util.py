"""Shared helpers for the parity tests."""
import numpy as np

from alego_amd import synth


def bits(a):
    """View float arrays as integer bit patterns for exact comparison (NaN-safe)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.nonzero(bits(got).reshape(-1) != bits(want).reshape(-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[:5]}: got {got.reshape(-1)[bad[:5]]} want {want.reshape(-1)[bad[:5]]}"


def quat_angle(q1, q2):
    """Rotation angle (rad) between two unit quaternions (w,x,y,z)."""
    d = abs(float(np.dot(q1, q2)))
    return 2.0 * np.arccos(min(1.0, d))


def scans(params, n, stream=0, flags=0, start=0):
    return [synth.scan(params, start + k, stream, flags) for k in range(n)]


def imu_stream(t0, t1, rate=100.0, yaw_rate=0.3, acc=(0.4, -0.2, 0.0), tilt=(0.02, -0.015)):
    """sensor_msgs/Imu samples [n, 11] (stamp, orientation w x y z, linear_acceleration, angular_velocity) of a platform that turns
    at `yaw_rate` rad/s with a small constant roll / pitch and accelerates by `acc` (body frame, gravity added as an IMU reports it)."""
    n = int(round((t1 - t0) * rate)) + 1
    out = np.zeros((n, 11))
    for i in range(n):
        t = t0 + i / rate
        r, p, y = tilt[0], tilt[1], yaw_rate * t
        cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
        q = (cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr)   # Rz Ry Rx
        g = 9.81
        out[i, 0] = t
        out[i, 1:5] = q
        out[i, 5:8] = (acc[0] - g * np.sin(p), acc[1] + g * np.cos(p) * np.sin(r), acc[2] + g * np.cos(p) * np.cos(r))
        out[i, 8:11] = (0.0, 0.0, yaw_rate)
    return out


def rank_deficient_plane_scene(seed=3):
    """A constructed LaserMapping input for the plane fit of laserMapping.cpp:425-452: a map frame (frame 0: ground, two walls, poles) that also holds isolated
    'rails' — five map points on a line, 0.3 - 0.45 m apart, nothing else within 1.5 m — and follow-up frames whose surf cloud has points next to the middle of
    every rail, so that their five nearest neighbours are exactly those five collinear points (d5^2 < 1).  Rail kinds: axis-aligned with exactly representable
    coordinates (two constant columns: rank 2 by any arithmetic), a general direction in f32, and near-collinear (1e-5 of lateral noise: rank 3, condition ~1e5).
    Returns (params_mods, frames): frames[i] = (corner_last, surf_last, outlier, odom7) in the lidar frame of frame i; odom7 = t xyz + q wxyz."""
    rng = np.random.default_rng(seed)
    mods = dict(lm_leaf_corner=0.2, lm_leaf_surf=0.2, lm_leaf_outlier=0.4, lm_every=1, min_keyframe_dist=0.05)
    g = np.mgrid[-12:12.01:0.5, -12:12.01:0.5].reshape(2, -1).T
    ground = np.c_[g, np.full(len(g), -1.7)] + rng.normal(0, 0.01, (len(g), 3))
    w = np.mgrid[-6:6.01:0.4, -1.5:2.01:0.4].reshape(2, -1).T
    wall_a = np.c_[np.full(len(w), 8.0), w] + rng.normal(0, 0.01, (len(w), 3))
    wall_b = np.c_[w[:, 0], np.full(len(w), -7.0), w[:, 1]] + rng.normal(0, 0.01, (len(w), 3))
    poles = []
    for px, py in ((5, 5), (-5, 4), (4, -5), (-6, -3), (2, 9), (-9, 1), (9, -2), (0, -10)):
        z = np.arange(-1.5, 2.01, 0.25)
        poles.append(np.c_[np.full(len(z), px), np.full(len(z), py), z] + rng.normal(0, 0.005, (len(z), 3)))
    poles = np.concatenate(poles)
    rails, mids = [], []
    k = 0
    for zi, z0 in enumerate((4.0, 6.5, 9.0)):
        for xi in range(-2, 3):
            for yi in range(-2, 3):
                c = np.array([xi * 3.0, yi * 3.0, z0])
                kind = k % 3
                if kind == 0:      # axis-aligned, coordinates on a 1/16 grid (exact in f32 and through the identity key pose)
                    a = (k // 3) % 3
                    pts = np.tile(np.round(c * 16) / 16 + 1 / 32, (5, 1)); pts[:, a] += (np.arange(5) - 2) * 0.3125
                elif kind == 1:    # a general direction, f32-rounded
                    d = rng.standard_normal(3); d /= np.linalg.norm(d)
                    pts = c + np.outer((np.arange(5) - 2) * 0.45, d)
                else:              # near-collinear
                    d = rng.standard_normal(3); d /= np.linalg.norm(d)
                    pts = c + np.outer((np.arange(5) - 2) * 0.45, d) + rng.normal(0, 1e-5, (5, 3))
                rails.append(pts.astype(np.float32).astype(np.float64)); mids.append(c)
                k += 1
    rails = np.concatenate(rails); mids = np.array(mids)

    def cloud(xyz, inten=0.0):
        out = np.zeros((len(xyz), 4), np.float32)
        out[:, :3] = xyz; out[:, 3] = inten
        return out

    def pose(i):   # the platform's true pose at frame i: a slow drive with a slight turn
        yaw = 0.012 * i
        return np.array([0.12 * i, 0.05 * i, 0.0]), yaw

    def to_lidar(xyz, i):
        t, yaw = pose(i)
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        return (xyz - t) @ R     # R^T (p - t)

    frames = []
    for i in range(4):
        t, yaw = pose(i)
        od = np.r_[t + (rng.normal(0, 0.01, 3) if i else 0), np.cos((yaw + (0.002 if i else 0)) / 2), 0.0, 0.0, np.sin((yaw + (0.002 if i else 0)) / 2)]
        if i == 0:
            surf = np.concatenate([ground, wall_a, wall_b, rails])
        else:   # the same world seen again (fresh noise) + query points next to the middle of every rail (lateral offset 2 - 15 cm)
            q = mids + rng.normal(0, 0.05, mids.shape)
            surf = np.concatenate([ground + rng.normal(0, 0.01, ground.shape), wall_a + rng.normal(0, 0.01, wall_a.shape), wall_b + rng.normal(0, 0.01, wall_b.shape), q])
        corner = poles + (rng.normal(0, 0.005, poles.shape) if i else 0)
        outl = np.c_[rng.uniform(-10, 10, (40, 2)), rng.uniform(-1, 1, 40)]
        frames.append((cloud(to_lidar(corner, i)), cloud(to_lidar(surf, i)), cloud(to_lidar(outl, i)), od))
    return mods, frames


# ---- LaserMapping's k-NN (lm_knn) at grid and rounding edges -----------------------------------------------------------------------------------

F32 = np.float32


def flim32(knn_max_dist):
    """the smallest f32 f with (double)f >= knn_max_dist: lm_knn's candidate limit"""
    f = F32(knn_max_dist)
    return np.nextafter(f, F32(np.inf)) if float(f) < knn_max_dist else f


def f32_dist2(map_xyz, q):
    """f32 squared distances of every map point to query q in the kernels' and FLANN's order, (dx^2 + dy^2) + dz^2"""
    m = np.asarray(map_xyz, F32)[:, :3]
    q = np.asarray(q, F32)[:3]
    d = m - q   # (elementwise f32: dx = q - m up to the sign, which the square drops)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def knn_brute_rows(map_xyz, queries, knn_max_dist):
    """numpy brute force of laserMapping.cpp:375-376 / :425-426: the five nearest map points of every query in ascending (f32 distance, index)
    order; the row is -1 x 5 when the map holds fewer than five points or the fifth is not closer than knn_max_dist (compared in f64)"""
    rows = np.full((len(queries), 5), -1, np.int32)
    if len(map_xyz) < 5:
        return rows
    idx = np.arange(len(map_xyz))
    for i, q in enumerate(np.asarray(queries, F32)):
        d = f32_dist2(map_xyz, q)
        o = np.lexsort((idx, d))[:5]
        if float(d[o[4]]) < knn_max_dist:
            rows[i] = o
    return rows


def lm_grid_cells_f32(raw_map_xyz, pts, knn_max_dist, gcap=1 << 20):
    """the uniform grid of lm_grid_build / grid_cell before it used integer cell coordinates: origin = the raw window's bounding-box minimum, cell =
    the smallest power of two >= sqrtf(knn_max_dist) (doubled while the box needs more than gcap cells), cell = floorf((x - ox) * inv) in f32,
    unclamped.  The scenes below use it to show that their premise holds: a neighbour the oracle finds lies outside the 27 cells of that formula."""
    raw = np.asarray(raw_map_xyz, F32)[:, :3]
    mn, mx = raw.min(axis=0), raw.max(axis=0)
    cell, need = F32(1.0), np.sqrt(F32(knn_max_dist))
    while cell < need:
        cell = F32(cell * 2)
    while True:
        g = [int(np.floor((mx[a] - mn[a]) / cell)) + 2 for a in range(3)]
        if g[0] * g[1] * g[2] <= gcap:
            break
        cell = F32(cell * 2)
    inv = F32(1.0) / cell
    p = np.asarray(pts, F32)[..., :3]
    return np.floor((p - mn) * inv).astype(np.int64), float(cell)


def lm_unit_cells_needed(raw_map_xyz):
    """cells of 1 m the raw box needs in lm_grid_build (floor(extent) + 2 per axis)"""
    raw = np.asarray(raw_map_xyz, F32)[:, :3]
    ext = raw.max(axis=0) - raw.min(axis=0)
    return int(np.prod([int(np.floor(e)) + 2 for e in ext]))


def _cloud(xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), F32)
    out[:, :3] = xyz
    return out


def _scene(kmd, leaf, map_xyz, q_xyz, **extra):
    """one key frame at the identity pose holding `map_xyz` as both its corner and its surf cloud (no outliers), then one mapping frame whose corner and
    surf clouds are `q_xyz` at the identity odometry: the queries reach lm_knn / the kd-tree unchanged (identity transforms are exact in f32 and f64),
    the maps are the voxel centroids of the key frame.  The solver budget is 0: these scenes are about the association (a handful of rows makes a
    degenerate least-squares problem); lm_blocks and the accepted lists are still compared."""
    mods = dict(knn_max_dist=float(kmd), lm_leaf_corner=float(leaf), lm_leaf_surf=float(leaf), lm_leaf_outlier=float(leaf), lm_every=1,
                lm_min_corner=1, lm_min_surf=1, lm_min_map_corner=1, lm_max_iters=0, min_keyframe_dist=1.0)
    m, q = _cloud(map_xyz), _cloud(q_xyz)
    return dict(mods=mods, keyframe=(np.zeros(6, F32), m, m, np.zeros((0, 4), F32)), frame=(q, q, np.zeros((0, 4), F32), np.array([0, 0, 0, 1.0, 0, 0, 0])), **extra)


def _axes(a):
    """coordinate order that puts the probe's axis at `a`"""
    return [a, (a + 1) % 3, (a + 2) % 3]


def _place(v, a):
    """v = (along, other1, other2) -> xyz with `along` on axis a"""
    out = [0.0, 0.0, 0.0]
    for k, ax in enumerate(_axes(a)):
        out[ax] = v[k]
    return out


# case 1: (box minimum ox, query q, fifth neighbour p) along one axis with cell c = sqrt(knn_max_dist): fl((p - q)^2) < c^2 but
# floorf((x - ox) / c) is 63 for q and 65 for p — the subtraction x - ox rounds across the binade boundary at 64 c
BINADE_TRIPLES = {1.0: (-53.062740325927734, 10.937256813049316, 11.937255859375), 4.0: (-116.13201904296875, 11.867976188659668, 13.867973327636719)}


def knn_binade_gap_scene(kmd):
    """A map whose raw box starts at (ox, ox, ox) and three probes, one per axis: a query at q on that axis (the other coordinates far from each other),
    four map points 0.25 m from it across the axis, and the fifth neighbour p on the axis at f32 d^2 just under knn_max_dist."""
    ox, q, p = (F32(v) for v in BINADE_TRIPLES[kmd])
    c = float(np.sqrt(kmd))
    pts, qs, probes = [[ox, ox, ox]], [], []
    for a in range(3):
        o1, o2 = float(F32(ox + (20 + 15 * a) * c)), float(F32(ox + (45 - 10 * a) * c))
        qs.append(_place((q, o1, o2), a))
        for d1, d2 in ((0.25, 0), (-0.25, 0), (0, 0.25), (0, -0.25)):
            pts.append(_place((q, o1 + d1, o2 + d2), a))
        pts.append(_place((p, o1, o2), a))
        probes.append((qs[-1], pts[-1], a))
    return _scene(kmd, 0.25, pts, qs, probes=probes)


# case 2: n copies of v summed in f32 and divided by n (pcl::CentroidPoint) give a centroid two ulps below v
CENTROID_V, CENTROID_N = 2659.309814453125, 23


def knn_centroid_below_box_scene(axis):
    """Five voxels of CENTROID_N identical points each at the window's minimum v on `axis` (1/128 m apart across it): their centroids lie two ulps below
    the raw box.  The query sits 1 - 1 ulp below the centroids on that axis: all five are within d^2 < 1, and the query's raw cell is -2."""
    v = F32(CENTROID_V)
    s = np.float32(1 / 128)
    ulp = np.spacing(v)
    c = _centroid(v, CENTROID_N)
    pts = []
    for k in (-2, -1, 0, 1, 2):
        pts += [_place((v, 5.0 + float(k * s), 7.0), axis)] * CENTROID_N
    q = F32(F32(c - F32(1)) + ulp)
    return _scene(1.0, 1 / 256, pts, [_place((q, 5.0, 7.0), axis)], centroid=c, v=v)


def _centroid(v, n):
    s = F32(0)
    for _ in range(n):
        s = F32(s + v)
    return F32(s / F32(n))


def _gate_offset(target, seed):
    """(dx, dy, dz), multiples of 2^-16, with fl(fl(dx^2 + dy^2) + dz^2) == target exactly"""
    rng = np.random.default_rng(seed)
    for _ in range(400000):
        dx, dz = F32(int(rng.integers(20000, 50000)) / 65536), F32(int(rng.integers(0, 20000)) / 65536)
        r = float(target) - float(dx * dx) - float(dz * dz)
        if r <= 0:
            continue
        b = int(np.sqrt(r) * 65536)
        for bb in range(b - 2, b + 3):
            dy = F32(bb / 65536)
            if F32(F32(dx * dx + dy * dy) + dz * dz) == target:
                return float(dx), float(dy), float(dz)
    raise AssertionError(f"no offset for {target!r}")


def knn_gate_scene(kmd):
    """Three probes: a query with four map points 0.25 m away and a fifth at f32 d^2 = flim - 1 ulp, flim, flim + 1 ulp (flim = the smallest f32 >=
    knn_max_dist).  Only the first is accepted."""
    fl = flim32(kmd)
    targets = (np.nextafter(fl, F32(0)), fl, np.nextafter(fl, F32(np.inf)))
    pts, qs, fifth = [], [], []
    for i, t in enumerate(targets):
        q = (4.0 * i + 1.0, 1.0, 1.0)
        qs.append(q)
        for d in ((0, 0, 0.25), (0, 0, -0.25), (-0.25, 0, 0), (0, -0.25, 0)):
            pts.append(np.add(q, d))
        pts.append(np.add(q, _gate_offset(t, 7 + i)))
        fifth.append((q, float(t), i == 0))
    return _scene(kmd, 0.25, pts, qs, fifth=fifth)


def knn_tie_scene(far):
    """A 6 x 6 x 6 lattice of 0.5 m (twice the leaf) and queries equidistant from 2 (edge midpoints), 4 (face centres) and 8 (cube centres) map points,
    plus queries one f32 ulp off the cube centres; `far` moves the scene about 4 km from the origin, where the f32 spacing is 2^-11 m."""
    o = np.array([4096.0, -4096.0, 4096.0]) if far else np.array([3.0, -2.0, 1.0])
    g = np.arange(6) * 0.5
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + o
    qs = []
    h = np.arange(5) * 0.5 + 0.25
    for x in h[::2]:
        for y in h[::2]:
            for z in h[::2]:
                c = o + (x, y, z)
                qs += [c, c + (0.25, 0, 0), c + (0, -0.25, 0.25), c + (0.25, 0.25, 0)]   # 8, 4, 2 ... equidistant points
                cc = F32(c)
                qs.append(np.nextafter(cc, F32(np.inf)))
                qs.append([np.nextafter(cc[0], F32(-np.inf)), cc[1], np.nextafter(cc[2], F32(np.inf))])
    return _scene(1.0, 0.25, lat, qs)


def knn_small_map_scene(n):
    """A map of n points (0.25 m apart, in one 0.5 m cube) and queries 0.5 - 1.5 cells outside its box on each of the six sides."""
    cube = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25], [0.25, 0.25, 0.25], [0.25, 0.25, 0], [0.5, 0, 0.25]])[:n] + (2.0, 3.0, 4.0)
    lo, hi = cube.min(axis=0), cube.max(axis=0)
    mid = (lo + hi) / 2
    qs = []
    for a in range(3):
        for t in (0.5, 0.75, 1.0, 1.25, 1.5):
            for side in (-1, 1):
                q = mid.copy()
                q[a] = (lo[a] - t) if side < 0 else (hi[a] + t)
                qs.append(q)
    return _scene(1.0, 0.125, cube, qs)


def knn_sparse_box_scene(extent, seed=11):
    """A sparse map whose box is `extent` metres (more unit cells than the handle's grid holds: lm_grid_build doubles the cell): eight clusters of
    a 0.25 m lattice and queries at their centres and 0.5 m beside them, plus the two box corners."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(extent, float)
    g = np.arange(3) * 0.25
    blob = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts, qs = [[0, 0, 0], list(ext)], []
    for _ in range(8):
        c = np.floor(rng.uniform(1, ext - 2) * 4) / 4
        pts += list(blob + c)
        qs += [c + 0.25, c + (0.25, 0.25, -0.5), c + (0.75, 0.25, 0.25), c + (-0.5, 0.5, 0.25)]
    return _scene(1.0, 0.25, pts, qs)


KNN_SCENES = ["binade_kmd1", "binade_kmd4", "centroid_x", "centroid_y", "centroid_z", "gate_1.0", "gate_0.7", "gate_1.1", "gate_2/3",
              "ties_near", "ties_far", "small_4", "small_5", "small_6"]


def knn_scene(name):
    kind, _, arg = name.partition("_")
    if kind == "binade":
        return knn_binade_gap_scene(float(arg[3:]))
    if kind == "centroid":
        return knn_centroid_below_box_scene("xyz".index(arg))
    if kind == "gate":
        return knn_gate_scene(2 / 3 if arg == "2/3" else float(arg))
    if kind == "ties":
        return knn_tie_scene(arg == "far")
    if kind == "small":
        return knn_small_map_scene(int(arg))
    raise KeyError(name)


def run_knn_scene(x, scene, device=False):
    """the scene's key frame, then its mapping frame, on an oracle or (device=True) a binding.Handle"""
    kp, c, s, ol = scene["keyframe"]
    x.lm_add_keyframe(kp, c, s, ol)
    qc, qs, qo, od = scene["frame"]
    if device:
        return x.lm_process(qc, qs, qo, dict(t=od[:3], q=od[3:]))
    return x.lm_process(qc, qs, qo, od)


def _row_of(cloud, xyz):
    hit = np.nonzero((cloud[:, :3] == F32(xyz)).all(axis=1))[0]
    assert hit.size == 1, (xyz, hit)
    return int(hit[0])


def assert_knn_scene_premise(name, scene, o):
    """What each scene is built to reach, recomputed from the oracle's own outputs of the scene (a later change must not make it vacuous)."""
    kmd = scene["mods"]["knn_max_dist"]
    assert o.get("lm_info")[1], f"{name}: the optimisation did not run"
    mc, qc, kc = o.get("lm_corner_map_ds"), o.get("lm_query_c"), o.get("lm_knn_c").reshape(-1, 5)
    raw = scene["keyframe"][1]
    if name.startswith("binade"):
        assert_bit_equal(mc, o.get("lm_surf_map_ds"), f"{name}: corner and surf maps")
        for q, pp, a in scene["probes"]:
            qi = _row_of(qc, q)
            row = kc[qi]
            assert row[4] >= 0, f"{name}: the oracle rejected the axis-{a} probe"
            p = mc[row[4]]
            assert np.array_equal(p[:3], F32(pp)), f"{name}: the fifth neighbour of the axis-{a} probe is not the planted point"
            cells, _ = lm_grid_cells_f32(raw, np.stack([qc[qi], p]), kmd)
            assert abs(cells[1, a] - cells[0, a]) >= 2, f"{name}: axis {a}: cells {cells.tolist()} are neighbours"
    elif name.startswith("centroid"):
        a = "xyz".index(name[-1])
        c, v = scene["centroid"], scene["v"]
        assert len(mc) == 5 and (mc[:, a] == c).all() and c < v - np.spacing(v), f"{name}: centroids {mc[:, a]} vs raw minimum {v!r}"
        assert (kc[0] >= 0).all(), f"{name}: the oracle rejected the query"
        cells, _ = lm_grid_cells_f32(raw, np.concatenate([qc[:1], mc]), kmd)
        assert cells[0, a] == -2 and (cells[1:, a] == -1).all(), f"{name}: cells {cells[:, a].tolist()}"
    elif name.startswith("gate"):
        for q, t, acc in scene["fifth"]:
            i = _row_of(qc, q)
            d = f32_dist2(mc, qc[i])
            assert np.sort(d)[4] == F32(t), f"{name}: probe {i}: fifth distance {np.sort(d)[4]!r} vs {t!r}"
            assert (kc[i, 0] >= 0) == acc, f"{name}: probe {i} (d5^2 = {t!r}) accepted {kc[i, 0] >= 0}"
    elif name.startswith("ties"):
        n_tied = 0
        for i, q in enumerate(qc):
            d = np.sort(f32_dist2(mc, q))
            n_tied += int(d[4] == d[5])
        assert (kc[:, 0] >= 0).all(), f"{name}: rejected queries"
        assert n_tied >= len(qc) // 2, f"{name}: only {n_tied} of {len(qc)} queries have a tie at the fifth neighbour"
    elif name.startswith("small"):
        n = int(name[-1])
        assert len(mc) == n
        acc = int((kc[:, 0] >= 0).sum())
        assert (acc == 0) if n < 5 else (0 < acc < len(qc)), f"{name}: {acc} of {len(qc)} queries accepted"
