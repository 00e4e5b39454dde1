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


# ---- PCL's "leaf size too small" rule in LaserMapping's VoxelGrids -----------------------------------------------------------------------------

INT_MAX = 2 ** 31 - 1


def pcl_dims(xyz, leaf):
    """pcl::VoxelGrid's grid size (dx, dy, dz) of a cloud, in its own f32 arithmetic: d = int64((max - min) * inv) + 1 with inv = 1.0f / leaf"""
    p = np.asarray(xyz, F32).reshape(-1, np.shape(xyz)[-1])[:, :3]
    inv = F32(1.0) / F32(leaf)
    ext = (p.max(axis=0) - p.min(axis=0)) * inv   # f32 throughout
    return tuple(int(e) + 1 for e in ext)


def pcl_passes(xyz, leaf):
    """True when pcl::VoxelGrid returns the cloud unchanged: dx * dy * dz > INT_MAX (never for an empty cloud)"""
    if len(xyz) == 0:
        return False
    dx, dy, dz = pcl_dims(xyz, leaf)
    return dx * dy * dz > INT_MAX


def voxel_grid_np(pts, leaf):
    """numpy restatement of pcl::VoxelGrid<PointXYZI>::applyFilter: the pass-through rule, then one centroid per voxel in ascending
    idx = i + j dx + k dx dy (stable), each the f32 sum of the voxel's points in input order divided by the count"""
    a = np.asarray(pts, F32)
    if len(a) == 0 or pcl_passes(a, leaf):
        return a.copy()
    inv = F32(1.0) / F32(leaf)
    xyz = a[:, :3]
    minb = np.floor(xyz.min(axis=0) * inv).astype(np.int64)
    maxb = np.floor(xyz.max(axis=0) * inv).astype(np.int64)
    div = maxb - minb + 1
    ijk = (np.floor(xyz * inv) - minb.astype(F32)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    out = []
    for key in np.unique(idx):
        members = order[idx[order] == key]
        s = np.zeros(4, F32)
        for i in members:
            s = s + a[i]
        out.append(s / F32(len(members)))
    return np.array(out, F32).reshape(-1, 4)


def _pass_world(rng):
    """a small static scene in map coordinates: ground, two walls, eight poles (corner), a few loose points (outlier)"""
    g = np.mgrid[-12:12.01:0.5, -12:12.01:0.5].reshape(2, -1).T
    ground = np.c_[g, np.full(len(g), -1.7)] + rng.normal(0, 0.01, (len(g), 3))
    w = np.mgrid[-6:6.01:0.4, -1.5:2.01:0.4].reshape(2, -1).T
    wall_a = np.c_[np.full(len(w), 8.0), w] + rng.normal(0, 0.01, (len(w), 3))
    wall_b = np.c_[w[:, 0], np.full(len(w), -7.0), w[:, 1]] + rng.normal(0, 0.01, (len(w), 3))
    poles = []
    for px, py in ((5, 5), (-5, 4), (4, -5), (-6, -3), (2, 9), (-9, 1), (9, -2), (0, -10)):
        z = np.arange(-1.5, 2.01, 0.25)
        poles.append(np.c_[np.full(len(z), px), np.full(len(z), py), z] + rng.normal(0, 0.005, (len(z), 3)))
    outl = np.c_[rng.uniform(-10, 10, (40, 2)), rng.uniform(-1, 1, 40)]
    return np.concatenate(poles), np.concatenate([ground, wall_a, wall_b]), outl


def _to_lidar(xyz, t, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return (np.asarray(xyz, float).reshape(-1, 3) - t) @ R   # R^T (p - t)


def _odom7(t, yaw):
    return np.r_[t, np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]


def _pass_mods(leaf_c, leaf_s, leaf_o, **extra):
    mods = dict(lm_leaf_corner=float(leaf_c), lm_leaf_surf=float(leaf_s), lm_leaf_outlier=float(leaf_o), lm_every=1, min_keyframe_dist=0.0)
    mods.update(extra)
    return mods


# scene 1: the window's box right at the rule.  INT_MAX = 2^31 - 1 is prime, so no box of three dimensions (and no f32 extent times inv, whose
# f32 values next to 2^31 are 128 apart) has it as its product: the largest reachable product below the rule is 2^31 - 2 = 49981 * 651 * 66.
# leaf 1/16 makes (max - min) * inv exact; "round" uses leaf 0.05 (inv = 20.0f) and an x extent whose exact product with inv lies below 32767
# while the f32 product rounds onto 32767, so that PCL's dx is 32768 and the product 2^31 (exact arithmetic: 2^31 - 65536, filtered).
PASS_BOUNDARY = {"below": (1 / 16, (49981, 651, 66), False), "above": (1 / 16, (32768, 1024, 64), True), "round": (0.05, (32768, 512, 128), True)}


def _round_extent(inv, k):
    """(x0, x1): f32 values with fl(fl(x1 - x0) * inv) == k although the exact (x1 - x0) * inv is below k"""
    inv = F32(inv)
    x0 = F32(-16.0)
    x1 = F32((k / float(inv)) + float(x0))
    for _ in range(64):   # (downwards from the nearest f32 of x0 + k / inv)
        e = F32(x1 - x0)
        if F32(e * inv) == F32(k) and float(e) * float(inv) < k and float(e) == float(x1) - float(x0):
            return float(x0), float(x1)
        if F32(e * inv) < F32(k):
            break
        x1 = np.nextafter(x1, F32(-np.inf))
    raise AssertionError(f"no extent rounds onto {k}")


def pass_boundary_scene(kind, maps):
    """Two key frames at the identity pose (lm_add_keyframe) that hold the scene plus one point at each corner of a box whose PCL grid is
    PASS_BOUNDARY[kind]; maps = "corner" (corner clouds), "surf" (min corner in a surf cloud, max corner in an outlier cloud: the surf map is
    surf + outlier) or "both".  Two mapping frames at the identity odometry follow; their key frames lie inside the box."""
    leaf, dims, passes = PASS_BOUNDARY[kind]
    rng = np.random.default_rng(21)
    inv = F32(1.0) / F32(leaf)
    lo, hi = [], []
    for a, d in enumerate(dims):
        if kind == "round" and a == 0:
            x0, x1 = _round_extent(inv, d - 1)
        else:
            e = F32((d - 1 + 0.5) / float(inv))   # half a cell past d - 1: the truncation is unambiguous
            x0 = float(F32(np.floor((0.15 if a == 2 else 0.0) * 32 - float(e) / 2 * 32) / 32))   # (centred on the scene)
            x1 = float(F32(x0 + e))
            assert float(F32(x1) - F32(x0)) == float(e)
        lo.append(x0); hi.append(x1)
    corner, surf, outl = _pass_world(rng)
    allp = np.concatenate([corner, surf, outl])
    assert (allp.min(0) > np.add(lo, 0.05)).all() and (allp.max(0) < np.subtract(hi, 0.05)).all(), "the scene must lie inside the box"
    leaf_c = leaf if maps in ("corner", "both") else 0.4
    leaf_s = leaf if maps in ("surf", "both") else 0.4
    kfs = []
    for k, anchor in enumerate((lo, hi)):
        c, s, o = corner.copy(), surf.copy(), outl.copy()
        if maps in ("corner", "both"):
            c = np.concatenate([c, [anchor]])
        if maps in ("surf", "both"):
            if k == 0:
                s = np.concatenate([s, [anchor]])
            else:
                o = np.concatenate([o, [anchor]])
        kfs.append((np.zeros(6, F32), _cloud(c), _cloud(s), _cloud(o)))
    frames = []
    for i in range(2):
        frames.append((_cloud(corner + rng.normal(0, 0.005, corner.shape)), _cloud(surf + rng.normal(0, 0.005, surf.shape)), _cloud(outl),
                       _odom7(np.zeros(3), 0.0)))
    expect = {i: (passes if maps != "surf" else False, passes if maps != "corner" else False) for i in range(2)}
    return dict(mods=_pass_mods(leaf_c, leaf_s, 0.4, recent_keyframe_num=4), keyframes=kfs, frames=frames, expect=expect, dims=dims,
                leaf=leaf, maps=maps)


def _moving_frames(n, rng, extra, pause=()):
    """n frames of the static scene seen from a platform that drives 0.41 m per frame (standing still at the frames in `pause`);
    extra[i] = (corner, surf, outlier) map points added to frame i"""
    corner, surf, outl = _pass_world(rng)
    frames, t, yaw = [], np.zeros(3), 0.0
    for i in range(n):
        if i and i not in pause:
            t = t + (0.4, 0.1, 0.0)
            yaw += 0.01
        ex = extra.get(i, (np.zeros((0, 3)),) * 3)
        c = np.concatenate([corner + rng.normal(0, 0.005, corner.shape), ex[0]])
        s = np.concatenate([surf + rng.normal(0, 0.005, surf.shape), ex[1]])
        o = np.concatenate([outl, ex[2]])
        frames.append((_cloud(_to_lidar(c, t, yaw)), _cloud(_to_lidar(s, t, yaw)), _cloud(_to_lidar(o, t, yaw)), _odom7(t, yaw)))
    return frames


def pass_window_scene(variant):
    """Enter, stay, leave: a 3-key-frame window, every mapping frame saves a key frame.  One frame holds a point 500 m along x, a later one a
    point 500 m along y (in all three clouds).  Neither frame alone crosses the rule at leaf 0.05 (~10^4 * 480 * 80 cells); a window holding
    both does (~10^4 * 10^4 * 80), so the maps pass through while both are in the window and are filtered again once the first has left.
      plain       X at frame 3, Y at frame 4: frames 5 and 6 pass, 7 - 9 filter
      quirk       the platform stands still at frame 3 (min_keyframe_dist 0.01: no key frame), X at 1, Y at 2: frame 3 passes with the window
                  {0, 1, 2}, frame 4 with the deque quirk's duplicate {1, 2, 2}, frames 5 - 8 filter
      correction  as plain, and after frame 5 every key pose is moved (lm_set_keypose), the window cleared and map -> odom corrected"""
    rng = np.random.default_rng(22)
    X = (np.array([[500.0, 0.0, 0.0]]),) * 3
    Y = (np.array([[0.0, 500.0, 0.0]]),) * 3
    if variant == "quirk":
        frames = _moving_frames(9, rng, {1: X, 2: Y}, pause=(3,))
        expect = {i: (i in (3, 4),) * 2 for i in range(2, 9)}   # (a window of one key frame is its own filtered map)
        mods = _pass_mods(0.05, 0.05, 0.05, recent_keyframe_num=3, min_keyframe_dist=0.01)
    else:
        frames = _moving_frames(10, rng, {3: X, 4: Y})
        expect = {i: (i in (5, 6),) * 2 for i in range(2, 10)}
        mods = _pass_mods(0.05, 0.05, 0.05, recent_keyframe_num=3)
    return dict(mods=mods, keyframes=[], frames=frames, expect=expect, correct_after=5 if variant == "correction" else None, variant=variant)


def _spread(rng, n, half=(100.0, 100.0, 15.0)):
    """n points spread over a 200 m x 200 m x 30 m box around the origin: its own grid at leaf 0.05 has 4000 * 4000 * 600 cells"""
    h = np.asarray(half)
    pts = rng.uniform(-h, h, (n, 3))
    pts[:2] = [-h, h]
    return pts


def pass_scan_scene(size):
    """The current scan's own clouds beyond the rule (downsampleCurrentScan: corner, surf and outlier, then laser_surf_total_): a key frame of
    the plain scene at the identity pose, then three mapping frames at the identity odometry (min_keyframe_dist 1: none saves a key frame) whose
    clouds also hold points spread over 200 m x 200 m x 30 m.  size "small": every cloud of at most 8192 points (vox_small); "big": the surf
    cloud and laser_surf_total_ above 8192 (vox_big)."""
    rng = np.random.default_rng(23 if size == "small" else 24)
    corner, surf, outl = _pass_world(rng)
    kf = (np.zeros(6, F32), _cloud(corner), _cloud(surf), _cloud(outl))
    ns = 2000 if size == "small" else 9000
    frames = []
    for i in range(3):
        c = np.concatenate([corner + rng.normal(0, 0.005, corner.shape), _spread(rng, 300)])
        s = np.concatenate([surf + rng.normal(0, 0.005, surf.shape), _spread(rng, ns)])
        o = np.concatenate([outl, _spread(rng, 1500)])
        frames.append((_cloud(c), _cloud(s), _cloud(o), _odom7(np.zeros(3), 0.0)))
    expect = {i: (False, False) for i in range(3)}
    return dict(mods=_pass_mods(0.05, 0.05, 0.05, recent_keyframe_num=3, min_keyframe_dist=1.0), keyframes=[kf], frames=frames, expect=expect,
                scan_pass=True, size=size)


def pass_keyframe_scene(size):
    """A single key frame beyond the rule: frame 3 of a moving run also holds points spread over 200 m x 200 m x 30 m in all three clouds, so
    its downsampled clouds are the raw ones and the key frame it saves crosses the rule on its own (the key-frame sort cannot order it).  With a
    3-key-frame window it is in the window at frames 4 - 6 (the maps pass through) and has left it at frame 7; frames 7 - 9 filter.
    size "small" / "big": the saved surf + outlier cloud of at most / more than 8192 points."""
    rng = np.random.default_rng(25 if size == "small" else 26)
    ns = 2000 if size == "small" else 9000
    frames = _moving_frames(10, rng, {3: (_spread(rng, 300), _spread(rng, ns), _spread(rng, 1500))})
    expect = {i: (i in (4, 5, 6),) * 2 for i in range(2, 10)}
    return dict(mods=_pass_mods(0.05, 0.05, 0.05, recent_keyframe_num=3), keyframes=[], frames=frames, expect=expect, kf_frame=3, size=size)


PASS_SCENES = [f"boundary_{k}_{m}" for k in PASS_BOUNDARY for m in ("corner", "surf", "both")] + \
    ["window_plain", "window_quirk", "window_correction", "scan_small", "scan_big", "keyframe_small", "keyframe_big"]


def pass_scene(name):
    kind, _, arg = name.partition("_")
    if kind == "boundary":
        k, m = arg.split("_")
        return pass_boundary_scene(k, m)
    if kind == "window":
        return pass_window_scene(arg)
    if kind == "scan":
        return pass_scan_scene(arg)
    if kind == "keyframe":
        return pass_keyframe_scene(arg)
    raise KeyError(name)


def assert_pass_scene_premise(name, scene, o, i):
    """What mapping frame i of the scene is built to reach, from the oracle's own outputs after that frame: each local map passes through
    (the filtered map is the raw concatenation, row for row) exactly where scene["expect"] says so; the boundary scenes' window has exactly the planned grid; the
    scan scenes' downsampled clouds are their inputs; the key-frame scene's saved frame crosses the rule on its own."""
    P = scene["mods"]
    if i not in scene["expect"]:
        return
    for m, (raw_name, ds_name, leaf) in enumerate((("lm_corner_map", "lm_corner_map_ds", P["lm_leaf_corner"]),
                                                   ("lm_surf_map", "lm_surf_map_ds", P["lm_leaf_surf"]))):
        raw, ds = o.get(raw_name), o.get(ds_name)
        want = scene["expect"][i][m]
        same = len(ds) == len(raw) and (bits(ds) == bits(raw)).all()   # (a sparse filtered map can keep every row, but not in the raw order)
        assert len(raw) > 0 and pcl_passes(raw, leaf) == want and same == want, \
            f"{name} frame {i}: {raw_name} of {len(raw)} points -> {len(ds)}, grid {pcl_dims(raw, leaf)}, expected pass-through {want}"
        if name.startswith("boundary") and scene["maps"] in (("corner", "both") if m == 0 else ("surf", "both")):
            assert pcl_dims(raw, leaf) == scene["dims"], f"{name} frame {i}: {raw_name} grid {pcl_dims(raw, leaf)} vs {scene['dims']}"
    if scene.get("scan_pass"):
        c, s, ol, _ = scene["frames"][i]
        for what, inp, leaf in (("lm_corner_ds", c, P["lm_leaf_corner"]), ("lm_surf_ds", s, P["lm_leaf_surf"]), ("lm_outlier_ds", ol, P["lm_leaf_outlier"])):
            assert pcl_passes(inp, leaf) and len(o.get(what)) == len(inp), f"{name} frame {i}: {what}"
        tot = o.get("lm_surf_total_ds")
        assert len(tot) == len(s) + len(ol), f"{name} frame {i}: laser_surf_total_ passes through"
        big = scene["size"] == "big"
        assert len(c) <= 8192 and len(ol) <= 8192 and (len(s) > 8192) == big and (len(tot) > 8192) == big, f"{name}: cloud sizes"
    if scene.get("variant") == "quirk" and i in (3, 4):   # frame 3 saves no key frame; frame 4's window is {1, 2, 2}
        nk = [len(o.lm_keyframe(k)[0]) for k in range(3)]
        assert o.get("lm_info")[11] == (3 if i == 3 else 4) and (i == 3 or len(o.get("lm_corner_map")) == nk[1] + 2 * nk[2]), f"{name} frame {i}: no duplicate"
    if name.startswith("keyframe") and i == scene["kf_frame"] + 1:
        kp = o.get("lm_keyposes").reshape(-1, 6)[scene["kf_frame"]]
        kc, ks, ko = o.lm_keyframe(scene["kf_frame"])
        assert pcl_passes(O_transform(kp, kc), P["lm_leaf_corner"]), f"{name}: the key frame's corner cloud does not cross the rule"
        kso = O_transform(kp, np.concatenate([ks, ko]))
        assert pcl_passes(kso, P["lm_leaf_surf"]) and (len(kso) > 8192) == (scene["size"] == "big"), f"{name}: the key frame's surf + outlier cloud"


def O_transform(pose6, pts):
    from oracle import oracle_py as O
    return O.transform_cloud(pose6, pts)


def pass_correction(keyposes):
    """the key-pose correction of the "correction" window scene (a rigid 'loop closure': 0.02 rad about z and a shift): the new f32 key poses
    and the 3 x 4 map -> odom correction"""
    c, s = np.cos(0.02), np.sin(0.02)
    rc = np.array([[c, -s, 0, 0.15], [s, c, 0, -0.1], [0, 0, 1, 0.02]])
    out = []
    for kp in np.asarray(keyposes).reshape(-1, 6):
        q = kp.astype(np.float64)
        q[:3] = rc[:, :3] @ q[:3] + rc[:, 3]
        q[5] += 0.02
        out.append(q.astype(F32))
    return out, rc


def run_pass_scene_oracle(o, scene, name):
    """the whole scene on an oracle, asserting its premise after every mapping frame; returns the number of frames whose maps passed through"""
    for kp, c, s, ol in scene["keyframes"]:
        o.lm_add_keyframe(kp, c, s, ol)
    npass = 0
    for i, (c, s, ol, od) in enumerate(scene["frames"]):
        o.lm_process(c, s, ol, od)
        assert_pass_scene_premise(name, scene, o, i)
        npass += int(any(scene["expect"].get(i, (False, False))))
        if i == scene.get("correct_after"):
            poses, rc = pass_correction(o.get("lm_keyposes"))
            for k, q in enumerate(poses):
                o.lm_set_keypose(k, q)
            o.lm_reset_window()
            o.lm_apply_correction(rc)
    return npass
