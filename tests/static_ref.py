"""The static-map rule in numpy scalars and Python integers, the reference of tests/test_static_math.py and
tests/test_static_map_gpu.py.  It shares no code with the library: a point's cell is f64 floor((x - origin) / cell), the classes are compared as
Python integers (no width to overflow) and the neighbourhood is an explicit loop over the cells of the grid within the radius."""
import math

import numpy as np

OCCUPIED, UNKNOWN, OUTSIDE, BELOW, NEIGHBOUR, REMOVED, VERDICTS = 0, 1, 2, 3, 4, 5, 6   # ALEGO_STATIC_*


def cell_class(hits, passes, occ):
    """100 / 0 / -1 of one cell; occ = (min_hits, hit_weight, pass_weight)"""
    h, p = int(hits), int(passes)
    if h >= int(occ[0]) and h * int(occ[1]) >= p * int(occ[2]):
        return 100
    return 0 if p > 0 else -1


def verdict(origin, cell, n, hits, passes, point, sensor_z=0.0, occ=(1, 2, 1), protect_radius=0, keep_below=None):
    """the verdict of one world point (f32 triple); hits / passes are (n2, n1, n0) arrays"""
    c = []
    for k in range(3):
        x = float(np.float32(point[k]))
        if not math.isfinite(x):
            return OUTSIDE
        q = (x - float(origin[k])) / float(cell[k])
        if not abs(q) <= 2.0 ** 30:
            return OUTSIDE
        c.append(math.floor(q))
    if any(c[k] < 0 or c[k] >= n[k] for k in range(3)):
        return OUTSIDE
    if keep_below is not None and float(np.float32(sensor_z)) < float(np.float32(keep_below)):
        return BELOW
    cls = cell_class(hits[c[2], c[1], c[0]], passes[c[2], c[1], c[0]], occ)
    if cls == 100:
        return OCCUPIED
    if cls == -1:
        return UNKNOWN
    r = int(protect_radius)
    for z in range(c[2] - r, c[2] + r + 1):
        for y in range(c[1] - r, c[1] + r + 1):
            for x in range(c[0] - r, c[0] + r + 1):
                if 0 <= x < n[0] and 0 <= y < n[1] and 0 <= z < n[2] and cell_class(hits[z, y, x], passes[z, y, x], occ) == 100:
                    return NEIGHBOUR
    return REMOVED


def mark(origin, cell, n, hits, passes, points, sensor_z=None, **rule):
    """(verdicts (m,) uint8, stats (VERDICTS,) int64) of the points (m, 3+)"""
    out, stats = np.zeros(len(points), np.uint8), np.zeros(VERDICTS, np.int64)
    for i, p in enumerate(points):
        v = verdict(origin, cell, n, hits, passes, p, 0.0 if sensor_z is None else sensor_z[i], **rule)
        out[i] = v
        stats[v] += 1
    return out, stats


# ---- the scene of both test files: a wall every key pose sees, a box each frame sees at another place ----
SCENE_GRID = ((-10.0, -2.0, -2.0), (0.5, 0.5, 0.5), (50, 30, 12))


def scene():
    """(key poses (6, 4), points (8 766, 4) with w = frame, is_box (8 766,)) of the scene; world coordinates, identity rotations"""
    kp = np.array([[k + 0.13, 0.11, 0.17, k] for k in range(6)], np.float32)
    wall = np.array([[-7.9 + 0.25 * i, 10.2, -0.93 + 0.25 * j] for i in range(85) for j in range(17)])
    pts, box = [], []
    for k in range(6):
        b = np.array([[k + 0.1 + dx, 5.2, 0.03 + dz] for dx in (0, .25, .5, .75) for dz in (.1, .35, .6, .85)])
        for cloud, flag in ((wall, False), (b, True)):
            pts.append(np.concatenate([cloud, np.full((cloud.shape[0], 1), k)], axis=1))
            box += [flag] * cloud.shape[0]
    return kp, np.concatenate(pts).astype(np.float32), np.array(box)
