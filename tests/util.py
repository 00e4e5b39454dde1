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


IP_OUTPUTS = ("seg", "ground", "col", "range", "ring_start", "ring_end", "outlier", "label_image")
IP_ORACLE_NAMES = (("seg", "seg_cloud"), ("ground", "seg_ground"), ("col", "seg_col"), ("range", "seg_range"), ("ring_start", "ring_start"),
                   ("ring_end", "ring_end"), ("outlier", "outlier"))


def ip_outputs(h, pts):
    """what ImageProjection hands on for one scan on a live handle: cloud_info, the outliers, the label image, and the range and flag images"""
    seg = h.ip_process(pts, want_labels=True)
    out = {k: np.array(seg[k]) for k in IP_OUTPUTS}
    out["range_img"] = h.debug_get("range_img").copy()
    out["flag_img"] = h.debug_get("flag_img") & 15   # ground, active, right-edge, down-edge (the multi-kernel paths keep working bits of their own above them)
    return out


def ip_run(p, pts):
    """ip_outputs of one scan on a handle of its own (created under whatever ALEGO_* switches the environment holds)"""
    from alego_amd import binding
    h = binding.Handle(p)
    out = ip_outputs(h, pts)
    h.close()
    return out


def assert_same_outputs(a, b, tag):
    for k in a:
        assert_bit_equal(a[k], b[k], f"{tag}: {k}")


def assert_ip_outputs_equal_oracle(out, o, tag):
    """ip_outputs of the scan the oracle `o` processed last, against its images and clouds"""
    assert_bit_equal(out["range_img"], o.get("range_img"), f"{tag}: range image")
    assert_bit_equal(out["flag_img"] & 1, o.get("ground_img"), f"{tag}: ground image")
    assert_bit_equal(out["label_image"], o.get("label_img"), f"{tag}: label image")
    for k, n in IP_ORACLE_NAMES:
        assert_bit_equal(out[k], o.get(n), f"{tag}: {n}")


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


def tall_cloud(n, rng):
    """n points (leaf 1) that pass PCL's INT_MAX rule on a grid of more than 2^32 cells: x and y are 0.9 or 1.1 (d = 1, but two cells), z
    spans [0, 2^30] on multiples of 128 (d = 2^30 + 1), so divb = (2, 2, 2^30 + 1) and PCL's wrapped u32 voxel ids need all 32 bits"""
    p = np.empty((n, 4), F32)
    p[:, 0] = rng.choice(F32([0.9, 1.1]), n)
    p[:, 1] = rng.choice(F32([0.9, 1.1]), n)
    p[:, 2] = rng.integers(0, 1 << 23, n).astype(F32) * F32(128)
    p[:2, 2] = [0, 1 << 30]
    p[:, 3] = rng.uniform(0, 1, n)
    assert not pcl_passes(p, 1.0) and np.prod(np.floor(p[:, :3].max(axis=0)).astype(np.int64) - np.floor(p[:, :3].min(axis=0)) + 1) > 2 ** 32
    return p


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


# ---- LaserOdometry's correspondence search (lo_assoc) at its edges --------------------------------------------------------------------------------

LO_R, LO_SPIKE = 20.0, 20.25   # ranges of the constructed segmented clouds: flat ground everywhere, a non-ground spike where a corner feature goes


def lo_assoc_brute(prev_less_flat, prev_less_sharp, flat, sharp, params6, P):
    """numpy restatement of laserOdometry.cpp:337-481 for every query: (surf rows (j, closest, idx2, idx3), corner rows (j, closest, idx2, -1)).
    closest is -1 on a rejected row, whose partial walk results stay: idx2 / idx3 of a surf row whose 1-NN passed the gate but whose walk found only
    one of them, idx2 = -1 and idx3 = -1 when the 1-NN did not pass.  1-NN: brute force over the f32 distance (dx^2 + dy^2) + dz^2, ties to the
    lowest index, accepted when (double)d < nearest_feature_dist.  Walk: up from closest + 1, then down from closest - 1, each direction ending at
    the first point whose int(intensity) lies beyond ring_window; pow(f32 difference, 2) summed in double, strict < against a running minimum
    that starts at nearest_feature_dist."""
    from oracle import oracle_py as O
    nfd, W = float(P.nearest_feature_dist), int(P.ring_window)

    def search(tg, qs, kind):
        tg = np.asarray(tg, F32).reshape(-1, 4)
        qs = np.asarray(qs, F32).reshape(-1, 4)
        rows = np.full((len(qs), 4), -1, np.int32)
        rows[:, 0] = np.arange(len(qs))
        if len(qs) == 0 or len(tg) == 0:
            return rows
        sel = O.transform_to_start(params6, qs)
        ring = tg[:, 3].astype(np.int64)   # (int)intensity: C truncation of a non-negative float
        for j, s in enumerate(sel):
            d = f32_dist2(tg, s)
            c = int(np.argmin(d))   # (first minimum: the lowest index)
            if not float(d[c]) < nfd:
                continue
            cs = ring[c]
            up = np.arange(c + 1, len(tg))
            stop = np.nonzero(ring[up] > cs + W)[0]
            up = up[:stop[0]] if stop.size else up
            dn = np.arange(c - 1, -1, -1)
            stop = np.nonzero(ring[dn] < cs - W)[0]
            dn = dn[:stop[0]] if stop.size else dn
            order = np.concatenate([up, dn]).astype(np.int64)   # the visiting order
            df = tg[order, :3] - s[:3]                           # f32 differences
            e = df.astype(np.float64) ** 2
            pd = (e[:, 0] + e[:, 1]) + e[:, 2]
            same = ring[order] == cs
            if kind == 0:
                cls2, cls3 = same, ~same
            else:
                cls2, cls3 = np.concatenate([ring[up] > cs, ring[dn] < cs]), np.zeros(len(order), bool)
            out = []
            for cls in (cls2, cls3):
                m = cls & (pd < nfd)
                if not m.any():
                    out.append(-1)
                    continue
                v = np.where(m, pd, np.inf)
                out.append(int(order[int(np.argmin(v))]))   # first minimum in visiting order: strict < keeps the first one seen
            i2, i3 = out
            ok = (i2 >= 0 and i3 >= 0) if kind == 0 else i2 >= 0
            rows[j] = (j, c if ok else -1, i2, i3 if kind == 0 else -1)
        return rows

    return search(prev_less_flat, flat, 0), search(prev_less_sharp, sharp, 1)


def lo_brute_detail(tg, sel, P, kind):
    """per query (already at transform_to_start): the f32 1-NN distances, the number of targets at the minimum, and the double walk distances of
    every candidate in the window by class — what the scene premises count"""
    tg = np.asarray(tg, F32).reshape(-1, 4)
    ring = tg[:, 3].astype(np.int64)
    out = []
    if len(tg) == 0:
        return out
    for s in np.asarray(sel, F32).reshape(-1, 4):
        d = f32_dist2(tg, s)
        c = int(np.argmin(d))
        e = (tg[:, :3] - s[:3]).astype(np.float64) ** 2
        pd = (e[:, 0] + e[:, 1]) + e[:, 2]
        out.append(dict(d=d, c=c, dmin=d[c], n_min=int((d == d[c]).sum()), ring=ring, pd=pd, cs=int(ring[c])))
    return out


def lo_grid_geometry(tg):
    """lo_grid_build's grid over a target cloud's (x, y) extent, restated: (gx, gy, csz) or None when there is no grid"""
    tg = np.asarray(tg, F32).reshape(-1, 4)
    n = len(tg)
    if n <= 0 or n > 65535:
        return None
    mn, mx = tg[:, :2].min(axis=0), tg[:, :2].max(axis=0)
    ext = mx - mn
    if not (ext[0] < F32(1e6) and ext[1] < F32(1e6)):
        return None
    csz = F32(1.0)
    for _ in range(24):
        gx, gy = int(np.floor(ext[0] / csz)) + 2, int(np.floor(ext[1] / csz)) + 2
        if gx * gy <= 4096:
            return gx, gy, float(csz)
        csz = F32(csz * 2)
    return None


def _sector_cover(L, nsec):
    """positions 0..L-1 of a ring's [startRingIndex, endRingIndex] that some sector of laserOdometry.cpp:177-178 visits (sp < ep)"""
    cov = np.zeros(max(L, 0), bool)
    S, E = 0, L - 1
    for j in range(nsec):
        sp = (S * (nsec - j) + E * j) // nsec
        ep = (S * (nsec - 1 - j) + E * (j + 1)) // nsec - 1
        if sp < ep:
            cov[sp:ep + 1] = True
    return cov


def _seg_from_rings(P, rings):
    """a segmented cloud from per-ring slot lists [(xyz, spike), ...] placed on the positions the sector split visits; 5 padding points on either
    side of every ring (ring_start = first + 5, ring_end = last - 5, as ImageProjection publishes them).  Non-spike points are ground with range
    LO_R (curvature 0: flat candidates, never corners); a spike is non-ground at LO_SPIKE with a column jump of 11 on both sides (no suppression,
    no occlusion marking reaches it), so it becomes a sharp / less_sharp feature.  Intensity = ring + col / 10000."""
    pts, gnd, col, rng_, rs, re_ = [], [], [], [], [], []
    far = np.array([4096.0, 4096.0, 4096.0], F32)
    for r in range(P.n_scan):
        slots = list(rings[r]) if r < len(rings) else []
        L = 0
        if slots:   # the shortest ring whose visited positions take the slots exactly, else the shortest that takes them all
            fit = [L for L in range(len(slots), len(slots) + 40) if _sector_cover(L, P.n_sectors).sum() == len(slots)]
            L = fit[0] if fit else next(L for L in range(len(slots), 10 * len(slots) + 40) if _sector_cover(L, P.n_sectors).sum() >= len(slots))
        cov = _sector_cover(L, P.n_sectors)
        seq = [(far, False)] * 5
        it = iter(slots)
        n_extra = int(cov.sum()) - len(slots)
        flat_slots = [s for s in slots if not s[1]]
        assert n_extra == 0 or flat_slots, f"ring {r}: {n_extra} visited positions left over and no flat target to repeat"
        for k in range(L):
            if cov[k]:
                s = next(it, None)
                if s is None:   # (a visited position beyond the slots: a second copy of a flat target, merged into its voxel)
                    s = flat_slots[n_extra % len(flat_slots)]
                    n_extra -= 1
                seq.append(s)
            else:
                seq.append((far, False))
        seq += [(far, False)] * 5
        rs.append(len(pts) + 5)
        re_.append(len(pts) + len(seq) - 6)
        c = 0
        for k, (xyz, spike) in enumerate(seq):
            if k > 0 and (spike or seq[k - 1][1]):
                c += 11
            elif k > 0:
                c += 1
            pts.append([xyz[0], xyz[1], xyz[2], F32(r) + F32(c) / F32(10000)])
            gnd.append(0 if spike else 1)
            col.append(c)
            rng_.append(LO_SPIKE if spike else LO_R)
        assert c < 65536
    n = len(pts)
    assert n <= P.n_scan * P.horizon_scan, (n, P.n_scan * P.horizon_scan)
    return dict(seg=np.asarray(pts, F32).reshape(-1, 4), ground=np.asarray(gnd, np.uint8), col=np.asarray(col, np.int32),
                range=np.asarray(rng_, F32), ring_start=np.asarray(rs, np.int32), ring_end=np.asarray(re_, np.int32), orientation=np.zeros(3, F32))


def lo_scene_params(name, geom):
    p = synth.default_params(*geom)
    p.lo_iters_surf = 0   # the corner search runs at exactly the forced parameters
    p.lo_iters_corner = 0
    for k, v in LO_SCENES_MODS.get(name.split(":")[0], {}).items():
        setattr(p, k, v)
    if ":" in name:
        k, v = name.split(":")[1].split("=")
        setattr(p, k, type(getattr(p, k))(float(v)))
    return p


def _target_rings(P, surf, corner):
    """surf / corner: {ring: [xyz, ...]} -> per-ring slot lists, each ring's corner spikes spread evenly among its flat targets"""
    rings = []
    for r in range(P.n_scan):
        s = [(np.asarray(x, F32), False) for x in surf.get(r, [])]
        c = [(np.asarray(x, F32), True) for x in corner.get(r, [])]
        out = list(s)
        for j, t in enumerate(c):
            out.insert((j + 1) * len(s) // (len(c) + 1) + j, t)
        rings.append(out)
    return rings


def _query_rings(P, ring_len=60, short_ring=None):
    """scan 1's profile: every ring ring_len positions of flat ground with a spike in every twelve (the sharp queries); xyz follow"""
    rings = []
    for r in range(P.n_scan):
        L = short_ring if (short_ring is not None and r == 0) else ring_len
        rings.append([(np.zeros(3, F32), k % 12 == 6) for k in range(L)])
    return rings


def build_lo_scene(name, geom):
    """the two segmented clouds of LO scene `name` on an n_scan x horizon sensor: scan 0 holds the targets, scan 1 the queries.  Feature selection
    reads only range / col / ground, so the picks of scan 1 are read from the oracle first and the queries' xyz placed on them afterwards
    (the scene's query lists, repeated until every pick has one)."""
    from oracle import oracle_py as O
    P = lo_scene_params(name, geom)
    spec = LO_SCENE_FNS[name.split(":")[0]](P)
    seg0 = _seg_from_rings(P, _target_rings(P, spec["surf"], spec.get("corner", {})))
    seg1 = _seg_from_rings(P, _query_rings(P, spec.get("ring_len", 60), spec.get("short_ring")))
    o = O.Oracle(P)
    o.set_seg(seg1)
    o.fe()
    fi, si = o.get("flat_idx"), o.get("sharp_idx")
    o.close()
    fq = np.asarray(spec["flat_q"], F32).reshape(-1, 3)
    sq = np.asarray(spec.get("sharp_q", spec["flat_q"]), F32).reshape(-1, 3)
    assert len(fi) >= len(fq) and len(si) >= len(sq), f"{name}: {len(fi)} flat / {len(si)} sharp picks for {len(fq)} / {len(sq)} queries"
    seg1["seg"][fi, :3] = fq[np.arange(len(fi)) % len(fq)]
    seg1["seg"][si, :3] = sq[np.arange(len(si)) % len(sq)]
    return dict(P=P, seg0=seg0, seg1=seg1, params6=np.asarray(spec.get("params6", np.zeros(6)), np.float64), spec=spec)


def run_lo_scene_oracle(sc):
    """scan 0, then scan 1 at the forced params6; returns the oracle (its clouds of scan 0 are in sc['less_flat'] / sc['less_sharp'])"""
    from oracle import oracle_py as O
    o = O.Oracle(sc["P"])
    o.set_seg(sc["seg0"])
    o.lo()
    sc["less_flat"], sc["less_sharp"] = o.get("less_flat"), o.get("less_sharp")
    o.set_lo_params(sc["params6"])
    o.set_seg(sc["seg1"])
    assert o.lo() == 1
    return o


def _put(d, P, r, *xyz):
    if 0 <= r < P.n_scan:
        d.setdefault(r, []).extend(np.asarray(x, F32) for x in xyz)


def lo_nn_ties(P):
    """queries at exactly equal f32 distance (0.25 or 9) from 2 - 4 targets: in one ring, in different rings (ascending and descending with the
    offset), and — in a band of its own — in one ring 40 fillers apart (different boxes); corner targets repeat the pattern without fillers"""
    NS, surf, corner, q = P.n_scan, {}, {}, []
    for k in range(24):
        c = np.array([8 * (k % 8) - 28, 10 * (k // 8) - 10, 0.25])
        a = 0.5 if k % 2 == 0 else 3.0
        offs = [(a, 0, 0), (-a, 0, 0), (0, a, 0), (0, -a, 0)][:2 + k % 3]
        for j, o in enumerate(offs):
            r = [k, k + 4 * j, k + NS - 1 - j, k + (j % 2)][k % 4] % NS
            _put(surf, P, r, c + o)
            _put(corner, P, r, c + o)
        q.append(c)
    for j in range(6):
        c = np.array([-80 + 32 * j, 30, 0.25])
        a = 3.0 if j % 2 else 0.5
        r = (5 * j + 2) % NS
        _put(surf, P, r, c + (0, -a, 0), c + (0, a, 0), *[c + (3.0 + 0.5 * i, 1.5 if a == 3.0 else 0.0, 0) for i in range(40)])
        q.append(c)
    return dict(surf=surf, corner=corner, flat_q=q)


def lo_nn_gate(P):
    """1-NN at f32 distance exactly nearest_feature_dist (rejected), one ulp below (accepted), one ulp above; each with two more targets at the same
    f32 distance (mirror images) in the same ring and the next, so that the walk can complete an accepted row"""
    nfd = P.nearest_feature_dist
    g = F32(nfd)
    lim = g if float(g) >= nfd else np.nextafter(g, F32(np.inf))   # the smallest f32 that is not < nfd
    surf, corner, q = {}, {}, []
    for i, t in enumerate([lim, np.nextafter(lim, F32(0)), np.nextafter(lim, F32(np.inf)), np.nextafter(np.nextafter(lim, F32(0)), F32(0))]):
        for rep in range(3):
            k = 4 * rep + i
            c = np.array([24.0 * (k % 4), 24.0 * (k // 4), 0.25])
            seed = 31 + k
            dx, dy, dz = _gate_offset(t, seed)
            while i == 0 and not dx * dx + dy * dy + dz * dz < nfd:   # at the gate: an exact (double) distance below it, so `<=` would accept
                seed += 1000
                dx, dy, dz = _gate_offset(t, seed)
            r = (3 * k + 1) % (P.n_scan - 1)
            _put(surf, P, r, c + (dx, dy, dz), c + (-dx, dy, dz))
            _put(surf, P, r + 1, c + (dx, -dy, dz))
            _put(corner, P, r, c + (dx, dy, dz))
            _put(corner, P, r + 1, c + (dx, -dy, dz))
            q.append(c)
    if float(lim) == nfd:   # 3-4-0 against an integer gate
        c = np.array([-24.0, 0.0, 0.25])
        _put(surf, P, 2, c + (3, 4, 0), c + (-3, 4, 0))
        _put(surf, P, 3, c + (3, -4, 0))
        q.append(c)
    return dict(surf=surf, corner=corner, flat_q=q)


def _walk_star(P, surf, corner, c, cs, kind):
    """closest at c + (0.25, 0, 0) in ring cs; kind 0: equal-distance candidates above and below it (ring cs: (+-1, +-1, 0); rings cs +- 1: (1, 1, 0));
    kind 1: only below (ring cs: (+-1, -1, 0); ring cs - 1: (+-1, 1, 0))"""
    _put(surf, P, cs, c + (0.25, 0, 0))
    _put(corner, P, cs, c + (0.25, 0, 0))
    if kind == 0:
        _put(surf, P, cs, c + (1, 1, 0), c + (-1, 1, 0), c + (1, -1, 0), c + (-1, -1, 0))
        _put(surf, P, cs + 1, c + (1, 1, 0), c + (-1, 1, 0))
        _put(surf, P, cs - 1, c + (1, 1, 0))
        _put(corner, P, cs + 1, c + (1, 1, 0), c + (-1, 1, 0))
        _put(corner, P, cs - 1, c + (1, 1, 0))
    else:
        _put(surf, P, cs, c + (1, -1, 0), c + (-1, -1, 0))
        _put(surf, P, cs - 1, c + (1, 1, 0), c + (-1, 1, 0))
        _put(corner, P, cs - 1, c + (1, 1, 0), c + (-1, 1, 0))


def lo_walk_ties(P):
    """equal double distances of second / third candidates: above against below (up wins), two on the way up (lower index wins), two on the way
    down (higher index wins), across two rings (class 3) and for corner one ring above against one below"""
    surf, corner, q = {}, {}, []
    for k in range(16):
        c = np.array([8.0 * (k % 8), 8.0 * (k // 8), 0.25])
        _walk_star(P, surf, corner, c, 1 + (3 * k) % (P.n_scan - 2), k % 2)
        q.append(c)
    return dict(surf=surf, corner=corner, flat_q=q)


def lo_walk_gate(P):
    """1-NN 0.0625 away; second / third candidates at double distance exactly nearest_feature_dist (3-4-0: rejected) and just below it
    (4 - 2^-20 for the 4: accepted)"""
    surf, corner, q = {}, {}, []
    for k in range(12):
        c = np.array([16.0 * (k % 6), 16.0 * (k // 6), 0.25])
        cs = 1 + (5 * k) % (P.n_scan - 2)
        y = 4.0 if k % 2 == 0 else 4.0 - 2.0 ** -20
        _put(surf, P, cs, c + (0.25, 0, 0), c + (3, y, 0))
        _put(surf, P, cs + 1, c + (-3, y, 0))
        _put(surf, P, cs - 1, c + (3, -y, 0))
        _put(corner, P, cs, c + (0.25, 0, 0))
        _put(corner, P, cs + 1, c + (-3, y, 0))
        _put(corner, P, cs - 1, c + (3, -y, 0))
        q.append(c)
    return dict(surf=surf, corner=corner, flat_q=q)


def lo_ring_window(P):
    """closest in ring cs (0, 1, mid, NS-2, NS-1); candidates at distance^2 4 in rings cs +- W (inside) and closer ones (1) in cs +- (W + 1)
    (outside); ring mid + 1 holds no target at all; ring NS - 3 holds one target (a surf closest without any idx2); a corner query with
    candidates only in its own ring"""
    NS, W = P.n_scan, P.ring_window
    mid = NS // 2
    surf, corner, q = {}, {}, []
    for k, cs in enumerate([0, 1, mid, NS - 2, NS - 1, mid - 1]):
        c = np.array([12.0 * k, 0.0, 0.25])
        _put(surf, P, cs, c + (0.25, 0, 0), c + (0, 0, 2.5))
        _put(corner, P, cs, c + (0.25, 0, 0))
        for sgn in (1, -1):
            for r, o in ((cs + sgn * W, (0, 2.0 * sgn, 0)), (cs + sgn * (W + 1), (sgn * 1.0, 0, 0))):
                if r != mid + 1 and r != NS - 3:
                    _put(surf, P, r, c + o)
                    _put(corner, P, r, c + o)
        q.append(c)
    c = np.array([0.0, 20.0, 0.25])   # the lone target of ring NS - 3
    _put(surf, P, NS - 3, c + (0.25, 0, 0))
    _put(surf, P, NS - 4, c + (0, 1, 0))
    q.append(c)
    c = np.array([12.0, 20.0, 0.25])  # corner: second candidates only in the closest's own ring
    _put(corner, P, 2, c + (0.25, 0, 0), c + (-1.0, 0, 0), c + (0, -2.0, 0))
    _put(surf, P, 2, c + (0, 0, 9.0))
    q.append(c)
    return dict(surf=surf, corner=corner, flat_q=q)


def lo_box_edges(P):
    """rings of 1, 31, 32, 33, 64 and 65 targets on lines along x (1 m apart, ring r at y = 0.5 r): queries at the first and last target, on
    either side of the 32-target box seams, and beyond the ends of the lines (the nearest point of the box is its corner: bound == distance)"""
    surf, q = {}, []
    sizes = [1, 31, 32, 33, 64, 65]
    for r, n in enumerate(sizes):
        y = 0.5 * r
        _put(surf, P, r, *[(float(i), y, 0.0) for i in range(n)])
        for i in sorted({0, n - 1, 30, 31, 32, 33, 63, 64}):
            if i < n:
                q.append((float(i), y, 0.25))
        q += [(-0.5, y, 0.25), (n - 0.5, y, 0.25), (-1.0, y, 0.0), (float(n), y, 0.0)]
    return dict(surf=surf, corner={}, flat_q=q)


LO_GRID_EXTENT = {"gc": 62.5, "double": 70.0, "csz8": 300.0, "none": 300.0}


def lo_grid_scene(P, kind):
    """a lattice of targets over [0, E] x [0, E] (E = 62.5: exactly 64 x 64 cells of 1 m, the full-grid sentinel; 70: one doubling; 300: cells of
    8 m; 'none': the same plus one target 1e6 m away, no grid).  Queries on cell boundaries, 0.5 / 1 / 1.5 cells outside every side, exactly one
    cell size from their nearest target in (x, y) (not settled by the grid), just inside that, and close in (x, y) but far in z"""
    E = LO_GRID_EXTENT[kind]
    g = lo_grid_geometry_of(E)
    s = E / 5
    surf, corner, q = {}, {}, []
    for i in range(6):
        for j in range(6):
            t, r = np.array([i * s, j * s, 0.0]), (i + 2 * j) % (P.n_scan - 1)
            _put(surf, P, r, t, t + (0, 0, 1.5))    # (the companions above and in the next ring let the walk accept the row)
            _put(surf, P, r + 1, t + (0, 0, -1.5))
            _put(corner, P, r, t)
            _put(corner, P, r + 1, t + (0, 0, -1.5))
    if kind == "none":
        _put(surf, P, 0, (1e6, 0.0, 0.0))
    csz = g[2] if g else 8.0
    for f in (0.5, 1.0, 1.5):
        for y in (0.0, 2 * s, E):
            q += [(-f * csz, y, 0.0), (E + f * csz, y, 0.0), (y, -f * csz, 0.0), (y, E + f * csz, 0.0)]
    for k in range(6):
        t = np.array([k * s, (5 - k) * s, 0.0])
        q += [t + (csz, 0, 0), t + (0, -csz, 0), t + (csz - 0.25, 0, 0), t + (0.5, 0, 30.0), t + (k * csz if k < 5 else 0.0, 0.0, 0.25)]
    return dict(surf=surf, corner=corner, flat_q=q)


def lo_grid_geometry_of(E):
    return lo_grid_geometry(np.array([[0.0, 0.0, 0.0, 0.0], [E, E, 0.0, 0.0]], F32))


def lo_grid_count(P, n):
    """at 64 x 2048: a less_flat cloud of exactly n targets (a 256 x 256 lattice of 1 m, cut to n) — 65535 has a grid (cells of 8 m),
    65536 has none and reads its boxes from HBM"""
    xs = np.arange(n)
    surf, q = {}, []
    per = -(-n // P.n_scan)
    for i in xs:
        _put(surf, P, int(i // per), (float(i % 256), float(i // 256), 0.0))
    rng = np.random.default_rng(n)
    q = np.round(rng.uniform(-2, 258, (300, 3)) * 16) / 16
    q[:, 2] = rng.uniform(-1, 1, 300)
    return dict(surf=surf, corner={}, flat_q=q, sharp_q=q[:150])


def lo_dense_random(P):
    """jittered 1 m lattice targets, queries near them under a generic rotation + translation; more queries than one sweep takes and not a multiple of 16"""
    rng = np.random.default_rng(5)
    surf, corner = {}, {}
    pts = []
    for i in range(24):
        for j in range(24):
            pts.append((i + rng.uniform(-0.25, 0.25), j + rng.uniform(-0.25, 0.25), rng.uniform(-0.5, 0.5)))
    pts = np.asarray(pts)
    rr = rng.integers(0, P.n_scan, len(pts))
    for p, r in zip(pts, rr):
        _put(surf, P, int(r), p)
    for p, r in zip(pts[::7], rr[::7]):
        _put(corner, P, int(r), p)
    p6 = np.array([0.31, -0.22, 0.05, 0.013, -0.021, 0.047])
    from oracle import oracle_py as O
    sel = rng.uniform(-1, 24, (200, 3))
    R = O.transform_to_start(p6, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]], F32))[:, :3].astype(np.float64)
    t = R[3]
    Rm = (R[:3] - t).T
    q = (np.linalg.solve(Rm, (sel - t).T)).T
    return dict(surf=surf, corner=corner, flat_q=q[:150], sharp_q=q[:100], params6=p6, ring_len=84, short_ring=23)


LO_SCENE_FNS = {"nn_ties": lo_nn_ties, "nn_gate": lo_nn_gate, "walk_ties": lo_walk_ties, "walk_gate": lo_walk_gate, "ring_window": lo_ring_window,
                "box_edges": lo_box_edges, "dense_random": lo_dense_random,
                **{f"grid_{k}": (lambda P, k=k: lo_grid_scene(P, k)) for k in LO_GRID_EXTENT},
                "grid_count_65535": lambda P: lo_grid_count(P, 65535), "grid_count_65536": lambda P: lo_grid_count(P, 65536)}
LO_SCENES_MODS = {"grid_gc": dict(nearest_feature_dist=100.0), "grid_double": dict(nearest_feature_dist=100.0),
                  "grid_csz8": dict(nearest_feature_dist=100.0), "grid_none": dict(nearest_feature_dist=100.0)}
LO_SCENES = ["nn_ties", "nn_gate", "nn_gate:nearest_feature_dist=0.49", "walk_ties", "walk_gate", "ring_window:ring_window=0", "ring_window:ring_window=1",
             "ring_window", "ring_window:ring_window=3", "ring_window:ring_window=100", "box_edges", "grid_gc", "grid_double", "grid_csz8", "grid_none",
             "dense_random"]
LO_SCENES_BIG = ["grid_count_65535", "grid_count_65536"]   # 64 x 2048 only: a 16 x 1800 scan cannot hold 65535 targets


def assert_lo_scene_premise(name, sc, o, rows):
    """What each LO scene is built to reach, recomputed from the oracle's own outputs (a later change must not make a scene vacuous).
    rows = lo_assoc_brute's (surf, corner) rows of the scene."""
    from oracle import oracle_py as O
    P, kind = sc["P"], name.split(":")[0]
    lf, ls = sc["less_flat"], sc["less_sharp"]
    nfd, W = P.nearest_feature_dist, P.ring_window
    sel_f = O.transform_to_start(sc["params6"], o.get("flat"))
    sel_s = O.transform_to_start(sc["params6"], o.get("sharp"))
    det_f, det_s = lo_brute_detail(lf, sel_f, P, 0), lo_brute_detail(ls, sel_s, P, 1)
    geo = lo_grid_geometry(lf)
    surf, corner = rows
    assert_bit_equal(o.get("lo_params_after_surf"), sc["params6"], f"{name}: params after the surf solve (lo_iters_surf = 0)")

    def n_where(det, rr, pred):
        return sum(1 for d, r in zip(det, rr) if pred(d, r))

    def walk_ties(det, rr, col):
        # accepted rows whose chosen walk candidate shares its double distance with another candidate of its class in the window
        out = 0
        for d, r in zip(det, rr):
            if r[1] < 0 or r[col] < 0:
                continue
            pd, ring, cs = d["pd"], d["ring"], d["cs"]
            win = (ring >= cs - W) & (ring <= cs + W)
            cls = (ring == cs) if (col == 2 and rr is surf) else ((ring != cs) if rr is surf else (ring != cs))
            m = win & cls & (pd == pd[r[col]])
            m[r[1]] = False
            out += int(m.sum() >= 2)
        return out

    if kind == "nn_ties":
        tied = [(d, r) for d, r in zip(det_f, surf) if d["n_min"] >= 2 and float(d["dmin"]) < nfd]
        assert len(tied) >= 8, f"{name}: {len(tied)} surf queries with an exact 1-NN tie"
        assert all(r[1] < 0 or r[1] == d["c"] for d, r in tied)
        g = 0.999 * geo[2] ** 2
        assert any(float(d["dmin"]) < g for d, _ in tied) and any(float(d["dmin"]) > g for d, _ in tied), f"{name}: ties on one search path only"
        assert n_where(det_s, corner, lambda d, r: d["n_min"] >= 2 and r[1] >= 0) >= 4, f"{name}: corner ties"
        assert n_where(det_f, surf, lambda d, r: d["n_min"] >= 2 and float(d["dmin"]) < nfd and np.ptp(d["ring"][np.nonzero(d["d"] == d["dmin"])[0]]) == 0
                       and np.ptp(np.nonzero(d["d"] == d["dmin"])[0]) > 32) >= 1, f"{name}: no accepted tie in one ring across boxes"
    elif kind == "nn_gate":
        g = F32(nfd)
        lim = g if float(g) >= nfd else np.nextafter(g, F32(np.inf))
        at = [r for d, r in zip(det_f, surf) if d["dmin"] == lim]
        below = [r for d, r in zip(det_f, surf) if d["dmin"] == np.nextafter(lim, F32(0))]
        assert at and all(r[1] < 0 and r[2] < 0 and r[3] < 0 for r in at), f"{name}: 1-NN at the gate not rejected"
        assert any(bool(((d["pd"] < nfd) & (d["d"] == lim)).sum() >= 3) for d in det_f if d["dmin"] == lim), f"{name}: the walk would accept a row at the gate"
        assert below and any(r[1] >= 0 for r in below), f"{name}: 1-NN one ulp below the gate never accepted"
        if float(g) != nfd:
            assert float(g) > nfd and any(d["dmin"] == g for d in det_f), f"{name}: f32(nearest_feature_dist) not reached"
    elif kind == "walk_ties":
        for what, det, rr, col in (("surf idx2", det_f, surf, 2), ("surf idx3", det_f, surf, 3), ("corner idx2", det_s, corner, 2)):
            assert walk_ties(det, rr, col) >= 4, f"{name}: {what}: too few ties among walk candidates"
        assert n_where(det_f, surf, lambda d, r: r[1] >= 0 and r[2] > r[1]) >= 4 and n_where(det_f, surf, lambda d, r: r[1] >= 0 and r[2] < r[1]) >= 4
    elif kind == "walk_gate":
        eq = n_where(det_f, surf, lambda d, r: float(d["dmin"]) < nfd and bool(((d["pd"] == nfd) & (np.abs(d["ring"] - d["cs"]) <= W)).any()))
        assert eq >= 4, f"{name}: {eq} queries with a walk candidate at exactly nearest_feature_dist"
        assert n_where(det_f, surf, lambda d, r: r[1] >= 0 and nfd - 1e-5 < d["pd"][r[3]] < nfd) >= 2, f"{name}: no third point just below the gate"
        assert n_where(det_s, corner, lambda d, r: r[1] >= 0 and nfd - 1e-5 < d["pd"][r[2]] < nfd) >= 2, f"{name}: no corner point just below the gate"
    elif kind == "ring_window":
        if W < P.n_scan:
            edge = n_where(det_f, surf, lambda d, r: r[3] >= 0 and abs(d["ring"][r[3]] - d["cs"]) == W and
                           bool(((np.abs(d["ring"] - d["cs"]) == W + 1) & (d["pd"] < d["pd"][r[3]])).any()))
            assert W == 0 or edge >= 2, f"{name}: no third point at cs +- W with a closer one at cs +- (W + 1)"
        assert n_where(det_f, surf, lambda d, r: d["cs"] in (0, P.n_scan - 1) and float(d["dmin"]) < nfd) >= 2
        assert n_where(det_f, surf, lambda d, r: float(d["dmin"]) < nfd and r[2] < 0 and (d["ring"] == d["cs"]).sum() == 1) >= 1, f"{name}: lone closest"
        assert n_where(det_s, corner, lambda d, r: float(d["dmin"]) < nfd and r[2] < 0) >= 1
    elif kind == "box_edges":
        cnt = np.bincount(lf[:, 3].astype(np.int64), minlength=6)[:6]
        assert cnt.tolist() == [1, 31, 32, 33, 64, 65], cnt
        base = np.concatenate([[0], np.cumsum(cnt)])
        pos = {int(r[1] - base[int(lf[r[1], 3])]) for r in surf if r[1] >= 0}
        assert {0, 30, 31, 32, 33, 63, 64} <= pos, f"{name}: closest positions in their rings {sorted(pos)}"
    elif kind.startswith("grid_count"):
        n = int(kind.split("_")[-1])
        assert len(lf) == n and (geo is None) == (n > 65535), (len(lf), geo)
        assert geo is None or geo[2] == 8.0
    elif kind.startswith("grid_"):
        want = {"gc": (64, 64, 1.0), "double": (37, 37, 2.0), "csz8": (39, 39, 8.0), "none": None}[kind[5:]]
        assert geo == want, f"{name}: grid {geo}"
        csz = 8.0 if geo is None else geo[2]
        assert n_where(det_f, surf, lambda d, r: r[1] >= 0 and float(d["dmin"]) == csz * csz) >= 2, f"{name}: no accepted 1-NN exactly one cell away"
        assert n_where(det_f, surf, lambda d, r: r[1] >= 0 and float(d["dmin"]) < 0.999 * csz * csz) >= 2
    elif kind == "dense_random":
        nq = len(surf)
        assert nq > 128 and nq % 16, f"{name}: {nq} surf queries"
        assert (surf[:, 1] >= 0).sum() >= 20 and (corner[:, 1] >= 0).sum() >= 5, ((surf[:, 1] >= 0).sum(), (corner[:, 1] >= 0).sum())


# ---- LaserMapping's merge-path local map (map_update / map_accum, kernels_map.hip) at its list and batch edges --------------------------------
#
# Recipe of every scene: 16 x 1800, lm_every 1, min_keyframe_dist 0, lm_max_iters 0, identity rotation, leaves that are powers of two.  Every mapping
# frame then saves a key frame at exactly the odometry pose whose clouds are the frame's own VoxelGrid-filtered inputs, and the window of frame i is
# the key frames max(0, i - K) .. i - 1: every run size and every position in the sorted voxel list follows from the construction, and the premise
# function proves it from the oracle's outputs.  Points sit on a lattice of voxels that is enumerated in key order (x fastest, then y, then z), so a
# lattice index orders like the voxel key; each point is its voxel's centre plus a jitter of +-0.2 leaf per axis (exact centres would make the f32
# sums blind to the summation order) with a random intensity.

MERGE_CONSTANTS = ("MU_FCAP", "MU_E", "MU_T", "MAP_R", "MA_JB", "MA_PT", "MA_T")
LAT_N, LAT_ORIGIN = 64, np.array([-32, -32, -1])   # lattice index -> cell (i % 64, (i / 64) % 64, i / 4096) + origin
VKEY_B = 1 << 20                                   # vgrid.h: a voxel key holds cells -2^20 .. 2^20 - 1 per axis


def merge_kernel_constants():
    """The constants of map_update / map_accum the scenes are built around, read from the kernels' source, so that a retune either moves the
    scenes with it or fails here; MA_BCAP (points per batch) is derived as the source derives it."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "a-lego-loam_amd", "csrc", "kernels_map.hip")
    with open(path) as f:
        src = f.read()
    out = {}
    for name in MERGE_CONSTANTS:
        found = re.findall(rf"^[ \t]*#define[ \t]+{name}[ \t]+(\d+)\b", src, re.M)
        assert len(found) == 1, f"kernels_map.hip: {len(found)} numeric #defines of {name}"
        out[name] = int(found[0])
    assert re.search(r"#define[ \t]+MA_BCAP[ \t]+\(MA_PT \* MA_T\)", src), "kernels_map.hip: MA_BCAP is no longer MA_PT * MA_T"
    out["MA_BCAP"] = out["MA_PT"] * out["MA_T"]
    return out


def _lat_cells(idx):
    idx = np.asarray(idx, np.int64).reshape(-1)
    return np.stack([idx % LAT_N, (idx // LAT_N) % LAT_N, idx // (LAT_N * LAT_N)], axis=1) + LAT_ORIGIN


def lat_points(idx, leaf, rng, quant=None):
    """one point per lattice index, shuffled; quant: the jitter is a multiple of `quant` metres (-1, 0 or 1 times) instead of uniform"""
    cell = _lat_cells(idx)
    jit = rng.integers(-1, 2, cell.shape) * (quant / leaf) if quant else rng.uniform(-0.2, 0.2, cell.shape)
    p = np.c_[(cell + 0.5 + jit) * leaf, rng.uniform(0, 100, len(cell))].astype(F32)
    return p[rng.permutation(len(p))]


def dense_points(vox, n, rng, leaf, sub):
    """n points on distinct `sub`-sized cells inside lattice voxel `vox` of size `leaf` (sub divides leaf)"""
    m = int(round(leaf / sub))
    cells = rng.choice(m ** 3, n, replace=False)
    c3 = np.stack([cells % m, (cells // m) % m, cells // (m * m)], axis=1)
    xyz = _lat_cells([vox]) * leaf + (c3 + 0.5 + rng.uniform(-0.2, 0.2, c3.shape)) * sub
    return np.c_[xyz, rng.uniform(0, 100, n)].astype(F32)


def vkeys(pts, leaf):
    """the voxel key of vgrid.h (z, y, x cells, 21 bits each) per point, from the f32 floor that pcl::VoxelGrid computes; the cells must be in range"""
    c = np.floor(np.asarray(pts, F32).reshape(-1, 4)[:, :3] * (F32(1.0) / F32(leaf))).astype(np.int64)
    assert (c >= -VKEY_B).all() and (c < VKEY_B).all()
    return ((c[:, 2] + VKEY_B) << 42) | ((c[:, 1] + VKEY_B) << 21) | (c[:, 0] + VKEY_B)


def _merge_mods(K, leaf_c=0.5, leaf_s=0.5, leaf_o=0.5, **extra):
    mods = dict(lm_leaf_corner=float(leaf_c), lm_leaf_surf=float(leaf_s), lm_leaf_outlier=float(leaf_o), lm_every=1, min_keyframe_dist=0.0,
                lm_max_iters=0, recent_keyframe_num=int(K))
    mods.update(extra)
    return mods


def _merge_frames(specs, mods, rng, quant=None):
    """specs[i] = dict(c=, s=, o=, t=): lattice indices (or ready n x 4 points) of the corner / surf / outlier cloud and the odometry translation"""
    frames = []
    for sp in specs:
        clouds = []
        for k, leaf in (("c", mods["lm_leaf_corner"]), ("s", mods["lm_leaf_surf"]), ("o", mods["lm_leaf_outlier"])):
            v = sp.get(k, ())
            clouds.append(v if isinstance(v, np.ndarray) and v.ndim == 2 else lat_points(v, leaf, rng, quant))
        frames.append((*clouds, _odom7(np.asarray(sp.get("t", (0.0, 0.0, 0.0)), float), 0.0)))
    return frames


_FILL_C = 8000 + np.arange(40)     # a line of 40 corner voxels
_FILL_S = 12288 + np.arange(200)   # a patch of 200 surf voxels on one z level
_FILL_O = 12288 + 3 * np.arange(20)


def merge_fcap_scene(C, rng):
    """surf map, K = 2: run sizes (surf + outlier points of a key frame) step through MU_FCAP - 96, MU_FCAP, MU_FCAP + 1 so that the (leaving, entering)
    pairs take map_update's fast path at its limit and its general path with one removal just beyond it.  Run k covers the voxels 1500 k .. 1500 k + 2999
    with one surf point each and spreads its outlier points over 1500 k .. 1500 k + 3199: the run that leaves shares about half its voxels with the one
    that stays, and the one that enters finds about half of its voxels in the list."""
    F = C["MU_FCAP"]
    sizes = [F, F + 1, F, F - 96, F + 1, F + 1, F + 1, F - 96, F, F]
    specs = [dict(c=_FILL_C, s=1500 * k + np.arange(3000), o=1500 * k + rng.choice(3200, n - 3000, replace=False)) for k, n in enumerate(sizes)]
    want = {i: dict(m=1, sizes=(sizes[i - 3], sizes[i - 1]), fast=max(sizes[i - 3], sizes[i - 1]) <= F, events=("dec_shared", "emptied", "inc_known", "new"))
            for i in range(3, len(sizes))}
    kinds = {(min(a, F), min(b, F)) if max(a, b) <= F else (a > F, b > F) for a, b in (w["sizes"] for w in want.values())}
    assert {(F, F), (True, False), (False, True), (True, True)} <= kinds, kinds
    mods = _merge_mods(2)
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng), want=want)


def merge_interval_scene(N, K, C, rng):
    """surf map, runs of at most MU_FCAP points: the update at frame K + 1 finds a list of exactly N voxels (list index k = lattice voxel 200 + 2 k) and
      empties U[0], U[N - 1], U[b - 1] and U[b] for the thread-interval boundaries b (MU_E and the last multiple of MU_E below N) and, for N >= 3 MU_E,
              all MU_E entries of thread 2
      inserts new voxels below U[0], above U[N - 1] and between U[b - 1] and U[b]
      keeps   a voxel that only the leaving and the entering run hold (count unchanged)
    K = 1: the entering run replaces the whole list.  K = 3 splits the staying voxels into two runs, the second of one voxel (N = 2 MU_FCAP + 1)."""
    E, FC = C["MU_E"], C["MU_FCAP"]
    v = lambda k: 200 + 2 * np.asarray(sorted(k), np.int64)
    bnds = sorted({b for b in (E, (N - 1) // E * E) if 0 < b < N})
    whole = set(range(2 * E, 3 * E)) if N >= 3 * E else set()
    r = 5
    must = {0, N - 1, r} | whole | {x for b in bnds for x in (b - 1, b)}
    cand = [k for k in range(0, N, 2) if k not in must]
    if K == 1:
        L, S = set(range(N)), set()
    else:
        L = must | set(cand[:max(0, FC - len(must))])
        S = (set(range(N)) - L) | ({k for k in cand if k % 4 == 0 and k in L} if N <= FC else set())
    assert len(L) <= FC and len(S) <= FC + (K == 3), (N, len(L), len(S))
    gone = (must - {r}) if K > 1 else (must - {r}) | {k for k in range(N) if k % 8 == 1}
    Ein = ({r} | {k for k in L - S if k % 8 == 2} | {k for k in S if k % 3 == 0}) if K > 1 else set(range(N)) - gone
    Ein -= gone
    new = [198, int(v([N - 1])[0]) + 2] + [int(v([b])[0]) - 1 for b in bnds]
    Ev = np.r_[v(Ein), new]
    assert len(Ev) <= FC
    runs = [v(L)] + ([v(S)] if K == 2 else [v(sorted(S)[:-1]), v(sorted(S)[-1:])] if K == 3 else []) + [Ev, v(range(0, N, 7))]
    specs = [dict(c=_FILL_C, s=run) for run in runs] + [dict(c=_FILL_C, s=runs[-1])]
    want = {K + 1: dict(m=1, nU_before=N, sizes=(len(L), len(Ev)), fast=True, emptied_has=sorted(gone), new_lb_has=[0, N] + bnds, readded_has=[r])}
    mods = _merge_mods(K)
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng), want=want)


def merge_chunk_scene(C, rng):
    """corner map, K = 2 (one point per voxel and run): the voxel count after the update is 1, MAP_R - 1, MAP_R, MAP_R + 1, 2 MAP_R and 2 MAP_R + 1;
    "both": voxels MAP_R - 1 and MAP_R (the last of map_accum's first work item and the first of its second) hold a point of either run; "split": one
    run ends in voxel MAP_R - 1 and the other begins in voxel MAP_R, in both window orders."""
    R = C["MAP_R"]
    a = np.arange
    kfs = [a(1), a(R - 1), a(R), a(R + 1), a(300, R + 1), np.array([k for k in range(2 * R) if k % 7 or k < 400 or k in (R - 1, R)]), a(400, 2 * R),
           a(2 * R + 1), a(R), a(R, 2 * R + 1), a(R)]
    specs = [dict(c=k, s=_FILL_S, o=_FILL_O) for k in kfs] + [dict(c=kfs[-1], s=_FILL_S, o=_FILL_O)]
    want = {i: dict(m=0, nU_after=len(set(kfs[max(0, i - 2)]) | set(kfs[i - 1]))) for i in range(1, len(specs))}
    for i in (5, 7, 8):
        want[i]["both"] = True
    for i in (10, 11):
        want[i]["split"] = True
    assert {1, R - 1, R, R + 1, 2 * R, 2 * R + 1} <= {w["nU_after"] for w in want.values()}
    mods = _merge_mods(2)
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng), want=want)


def merge_dense_scene(K, C, rng):
    """surf leaf 2, outlier leaf 1/16: every frame's outlier cloud puts 3000 points on distinct 1/16 cells of ONE surf voxel, so the key frame keeps them
    all and that voxel's piece of every run exceeds map_accum's batch of MA_BCAP points: the voxel's run is cut into sub-pieces and its thread carries
    the sum across batches.  K = 10: more than MA_JB runs feed the chunk."""
    n, D = 3000, 100
    assert n > 2 * C["MA_BCAP"] and (K <= 2 or K > C["MA_JB"])
    mods = _merge_mods(K, leaf_s=2.0, leaf_o=1 / 16)
    specs = [dict(c=_FILL_C, s=np.arange(300), o=dense_points(D, n, rng, 2.0, 1 / 16)) for _ in range(K + 3)]
    want = {i: dict(m=1, nU_after=300, runs=min(i, K), max_voxel_run=n + 1, kraw=min(i, K) * (300 + n)) for i in range(1, K + 3)}
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng), want=want)


def merge_dense_cut_scene(C, rng):
    """as dense, K = 1 (the window is one run, so batch offsets are offsets into the sorted run): ten single-point voxels, then three adjacent voxels
    X, Y, Z whose lengths put the voxel changes at MA_BCAP - 1, MA_BCAP and MA_BCAP + 1 (layout A: the batch cut falls one after, exactly on and one
    before a change) or at MA_BCAP - 1, 2 MA_BCAP and 3 MA_BCAP + 1 (layout B: the same three cases at three successive cuts of long voxel runs)."""
    B, X = C["MA_BCAP"], 10
    mods = _merge_mods(1, leaf_s=2.0, leaf_o=1 / 16)
    surf = np.r_[np.arange(X), np.arange(X + 3, 300)]
    lay = {"A": ((B - 1 - X, 1, 1), [B - 1, B, B + 1]), "B": ((B - 1 - X, B + 1, B + 1), [B - 1, 2 * B, 3 * B + 1])}
    specs, want = [], {}
    for i, which in enumerate("ABABA"):
        lens, changes = lay[which]
        specs.append(dict(c=_FILL_C, s=surf, o=np.concatenate([dense_points(X + j, n, rng, 2.0, 1 / 16) for j, n in enumerate(lens)])))
        want[i + 1] = dict(m=1, nU_after=300, runs=1, changes_has=changes, kraw=297 + sum(lens))
    specs.append(specs[-1])
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng), want=want)


def merge_empty_scene(C, rng):
    """K = 2, frames without any corner point: windows of zero-length runs, an empty corner map (no work item), the step from empty to non-empty (an
    empty list refuses the fast path), a zero-length run that enters on the fast path, and the step back to an empty list"""
    sizes = [0, 0, 0, 40, 40, 0, 0, 0, 30, 30]
    specs = [dict(c=50 * k + np.arange(n), s=_FILL_S, o=_FILL_O) for k, n in enumerate(sizes)]
    want = {}
    for i in range(1, len(sizes)):
        prev, cur = sizes[max(0, i - 3):i - 1], sizes[max(0, i - 2):i]
        want[i] = dict(m=0, kraw=sum(cur), nU_before=sum(prev), nU_after=sum(cur))
    want[4].update(fast=False, sizes=(0, 40)); want[6].update(fast=True, sizes=(40, 0)); want[7].update(fast=True, sizes=(40, 0)); want[9].update(fast=False)
    mods = _merge_mods(2)
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng), want=want)


def merge_far_scene(side, C, rng):
    """leaf 0.5 (cell 2^20 begins at 524288 m, where f32 values are 1/16 apart: the jitter is -1/16, 0 or 1/16), K = 2: compact clouds (64 x 8 x 1 surf
    cells, a few outliers, five corner points: below lm_min_corner, so no association at coordinates where lattice points tie) that the odometry
    translation places so that the frame's extreme x cell is the given one.  side +1: windows whose largest x cell is 2^20 - 1 (in range), 2^20, and
    2^20 + 31 (the window straddles the limit); side -1: smallest x cell -2^20 (in range), -2^20 - 1, -2^20 - 32.  want[i]["raises"]: the window of
    frame i has a cell that the 21-bit voxel key cannot hold."""
    P = VKEY_B
    ext = [P - 1, P - 1, P - 1, P, P, P + 31, P + 31, P - 1, P - 1, P - 1, P - 1] if side > 0 else [-P, -P, -P, -P - 1, -P - 1, -P - 32, -P - 32, -P, -P, -P, -P]
    local = 31 if side > 0 else -32
    mods = _merge_mods(2)
    specs = [dict(c=np.arange(5), s=np.arange(512), o=3 * np.arange(60), t=((e - local) * 0.5, 0.0, 0.0)) for e in ext]
    want = {}
    for i in range(1, len(ext)):
        w = ext[max(0, i - 2):i]
        x = max(w) if side > 0 else min(w)
        want[i] = dict(m=1, far_x=x, raises=not (-P <= x <= P - 1))
    assert {w["far_x"] for w in want.values()} == set(ext)
    return dict(mods=mods, frames=_merge_frames(specs, mods, rng, quant=1 / 16), want=want, far=side)


MERGE_SCENES = ["fcap", "interval_one_thread", "interval_three_threads", "interval_round", "interval_round_plus_one", "interval_replace",
                "chunk", "dense_k1", "dense_k2", "dense_k10", "dense_cut", "empty", "far_pos", "far_neg"]


def merge_scene(name, C=None):
    C = C or merge_kernel_constants()
    rng = np.random.default_rng(31 + MERGE_SCENES.index(name))
    E, T = C["MU_E"], C["MU_T"]
    if name == "fcap":
        sc = merge_fcap_scene(C, rng)
    elif name.startswith("interval"):
        N, K = {"one_thread": (E, 2), "three_threads": (3 * E, 2), "round": (T * E, 2), "round_plus_one": (T * E + 1, 3), "replace": (3 * E, 1)}[name[9:]]
        sc = merge_interval_scene(N, K, C, rng)
    elif name == "chunk":
        sc = merge_chunk_scene(C, rng)
    elif name == "dense_cut":
        sc = merge_dense_cut_scene(C, rng)
    elif name.startswith("dense"):
        sc = merge_dense_scene(int(name[7:]), C, rng)
    elif name == "empty":
        sc = merge_empty_scene(C, rng)
    elif name.startswith("far"):
        sc = merge_far_scene(1 if name == "far_pos" else -1, C, rng)
    else:
        raise KeyError(name)
    sc.update(keyframes=[], K=sc["mods"]["recent_keyframe_num"], C=C)
    assert max(sum(len(x) for x in f[:3]) for f in sc["frames"]) <= 15000
    return sc


def merge_window_facts(scene, o, i, m):
    """What map_update and map_accum meet at mapping frame i (>= 1) for map m (0 corner, 1 surf), from the oracle's key frames and maps alone: the runs
    of the previous and of the current window, the voxel list before and after, and every list event of the update."""
    K, C = scene["K"], scene["C"]
    leaf = scene["mods"]["lm_leaf_surf" if m else "lm_leaf_corner"]
    raw, ds = o.get("lm_surf_map" if m else "lm_corner_map"), o.get("lm_surf_map_ds" if m else "lm_corner_map_ds")
    run = {}
    for k in range(max(0, i - 1 - K), i):
        kc, ks, ko = o.lm_keyframe(k)
        run[k] = kc if m == 0 else np.concatenate([ks, ko])
    prev, cur = list(range(max(0, i - 1 - K), i - 1)), list(range(max(0, i - K), i))
    f = dict(kraw=len(raw), nds=len(ds), run_sizes=[len(run[k]) for k in cur])
    assert len(raw) == sum(f["run_sizes"]), f"frame {i} map {m}: raw map of {len(raw)} points vs runs {f['run_sizes']}"
    if scene.get("far"):
        return f
    cat = np.concatenate([run[k] for k in cur])
    assert (bits(cat) == bits(raw)).all(), f"frame {i} map {m}: the window is not key frames {cur} at the zero pose"
    keys = {k: vkeys(run[k], leaf).tolist() for k in run}
    setof = lambda ids: set().union(*[set(keys[k]) for k in ids]) if ids else set()
    Ub, Ua = sorted(setof(prev)), sorted(setof(cur))
    leaving, entering, staying = [k for k in prev if k not in cur], [k for k in cur if k not in prev], [k for k in cur if k in prev]
    kL, kE, kS = setof(leaving), setof(entering), setof(staying)
    pos = {key: p for p, key in enumerate(Ub)}
    import bisect
    f.update(nU_before=len(Ub), nU_after=len(Ua), chunks=-(-len(Ua) // C["MAP_R"]), runs=sum(1 for k in cur if len(run[k])),
             sizes=(len(run[leaving[0]]) if len(leaving) == 1 else None, len(run[entering[0]]) if len(entering) == 1 else None),
             emptied=sorted(pos[key] for key in set(Ub) - set(Ua)), new_lb=sorted(bisect.bisect_left(Ub, key) for key in set(Ua) - set(Ub)),
             readded=sorted(pos[key] for key in (kL & kE) - kS), dec_shared=len(kL & kS), inc_known=len(kE & (kS | kL) & set(Ub)))
    f["new"] = len(f["new_lb"])
    f["fast"] = len(Ub) > 0 and len(leaving) <= 1 and len(entering) <= 1 and max(f["sizes"][0] or 0, f["sizes"][1] or 0) <= C["MU_FCAP"]
    cnt = [np.unique(keys[k], return_counts=True)[1].max() if len(keys[k]) else 0 for k in cur]
    f["max_voxel_run"] = int(max(cnt)) if cnt else 0
    if cur and len(keys[cur[0]]):
        ks0 = sorted(keys[cur[0]])
        f["changes"] = [j for j in range(1, len(ks0)) if ks0[j] != ks0[j - 1]]
    R = C["MAP_R"]
    if len(Ua) > R and len(cur) == 2:
        a, b = keys[cur[0]], keys[cur[1]]
        f["both"] = all(Ua[x] in set(a) and Ua[x] in set(b) for x in (R - 1, R))
        f["split"] = (max(a) == Ua[R - 1] and min(b) == Ua[R]) or (max(b) == Ua[R - 1] and min(a) == Ua[R])
    return f


def assert_merge_scene_premise(name, scene, o, i):
    """Frame i of the scene reaches what it was built for, proven from the oracle's outputs after that frame (key-frame clouds, raw and filtered
    maps); returns the recorded facts of the map the scene is about (None at a frame without a window)."""
    if i == 0:
        assert len(o.get("lm_corner_map")) == 0 and len(o.get("lm_surf_map")) == 0
        return None
    P = scene["mods"]
    for m, (raw_name, ds_name, leaf) in enumerate((("lm_corner_map", "lm_corner_map_ds", P["lm_leaf_corner"]), ("lm_surf_map", "lm_surf_map_ds", P["lm_leaf_surf"]))):
        assert not pcl_passes(o.get(raw_name), leaf), f"{name} frame {i}: {raw_name} passes through"
    assert o.get("lm_info")[11] == i + 1, f"{name} frame {i}: {o.get('lm_info')[11]} key frames"
    want = scene["want"].get(i, dict(m=1))
    f = merge_window_facts(scene, o, i, want["m"])
    tag = f"{name} frame {i} map {want['m']}: "
    if scene.get("far"):
        raw = o.get("lm_surf_map")
        cx = np.floor(raw[:, 0] * (F32(1.0) / F32(P["lm_leaf_surf"]))).astype(np.int64)
        f["far_x"] = int(cx.max() if scene["far"] > 0 else cx.min())
        f["refused"] = []   # per map (corner, surf): the window has a cell that the voxel key cannot hold
        for r, leaf in ((o.get("lm_corner_map"), P["lm_leaf_corner"]), (raw, P["lm_leaf_surf"])):
            c3 = np.floor(r[:, :3] * (F32(1.0) / F32(leaf))).astype(np.int64)
            f["refused"].append(bool((c3 < -VKEY_B).any() or (c3 > VKEY_B - 1).any()))
        f["raises"] = any(f["refused"])
        assert max(pcl_dims(raw, P["lm_leaf_surf"])) <= 2 * LAT_N, tag + f"window grid {pcl_dims(raw, P['lm_leaf_surf'])} is not compact"
    else:
        assert f["nds"] == f["nU_after"], tag + f"{f['nds']} filtered points vs {f['nU_after']} occupied voxels"
    for k, w in want.items():
        if k == "m":
            continue
        if k.endswith("_has"):
            assert set(w) <= set(f[k[:-4]]), tag + f"{k[:-4]} = {f[k[:-4]][:40]} lacks {sorted(set(w) - set(f[k[:-4]]))}"
        elif k == "events":
            assert all(f[e] > 0 if not isinstance(f[e], list) else len(f[e]) > 0 for e in w), tag + f"events {[(e, f[e] if not isinstance(f[e], list) else len(f[e])) for e in w]}"
        elif k == "max_voxel_run":
            assert f[k] >= w, tag + f"{k} = {f[k]} < {w}"
        else:
            assert f[k] == w, tag + f"{k} = {f[k]} vs planned {w}"
    return f


def run_merge_scene_oracle(o, scene, name):
    """the whole scene on an oracle: every premise, and the oracle's filtered maps against voxel_grid_np of its raw windows, bit for bit; returns the
    recorded facts per frame"""
    P = scene["mods"]
    facts = {}
    for i, (c, s, ol, od) in enumerate(scene["frames"]):
        o.lm_process(c, s, ol, od)
        facts[i] = assert_merge_scene_premise(name, scene, o, i)
        for raw_name, ds_name, leaf in (("lm_corner_map", "lm_corner_map_ds", P["lm_leaf_corner"]), ("lm_surf_map", "lm_surf_map_ds", P["lm_leaf_surf"])):
            assert_bit_equal(o.get(ds_name), voxel_grid_np(o.get(raw_name), leaf), f"{name} frame {i}: {ds_name} vs the numpy VoxelGrid")
    return facts


# ---- the opt-in siblings of LaserMapping's registration (tests/test_regcov_gpu.py, tests/test_remap_gpu.py) ----------------------------------------

LI_NCUR_C, LI_NTOTAL_DS = 19, 23


def reg_params(**kw):
    p = synth.default_params(16, 1800)
    p.min_keyframe_dist = 0.03   # (squared) the synthetic platform moves 0.2 m per mapping frame: every one of them saves a key frame
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_REG_SCANS = {}


def reg_scan(k, stream=0):
    if (k, stream) not in _REG_SCANS:
        _REG_SCANS[(k, stream)] = synth.scan(reg_params(), k, stream)
    return _REG_SCANS[(k, stream)]


def assert_same_record(a, b, what, ints, floats):
    for k in ints:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in floats:
        assert_bit_equal(np.asarray(a[k]), np.asarray(b[k]), f"{what}: {k}")


def reg_rows_of_frame(h, slot=0):
    """lm_info and the accepted rows (edges (n, 9), planes (m, 7)) of the slot's last mapping frame as lm_fit left them"""
    p = h.params
    gi = h.debug_get("lm_info", slot=slot)
    kf_cap_c = p.n_less_sharp * p.n_sectors * p.n_scan
    blocks = h.debug_get("lm_blocks", slot=slot).reshape(-1, 8)
    qc, qs = h.debug_get("lm_corner_ds", slot=slot), h.debug_get("lm_surf_total_ds", slot=slot)
    assert len(qc) == gi[LI_NCUR_C] and len(qs) == gi[LI_NTOTAL_DS]
    bc, bs = blocks[:len(qc)], blocks[kf_cap_c:kf_cap_c + len(qs)]
    mc, ms = bc[:, 7] == 2.0, bs[:, 7] == 3.0
    assert ((bc[:, 7] == 0.0) | mc).all() and ((bs[:, 7] == 0.0) | ms).all()
    E = np.concatenate([bc[mc, 0:6], qc[mc, :3].astype(np.float64)], 1)
    S = np.concatenate([bs[ms, 0:3], bs[ms, 6:7], qs[ms, :3].astype(np.float64)], 1)
    return gi, E, S


def lm_observables(h, slot):
    return dict(info=h.debug_get("lm_info", slot=slot), state=h.debug_get("lm_state", slot=slot), keyposes=h.debug_get("lm_keyposes", slot=slot),
                cmap=h.debug_get("lm_corner_map_ds", slot=slot), smap=h.debug_get("lm_surf_map_ds", slot=slot), window=h.debug_get("lm_window", slot=slot))
