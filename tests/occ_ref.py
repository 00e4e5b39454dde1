"""An exact rational voxel traversal, the reference of tests/test_occ_math.py.  It shares no code with the library: every crossing of a cell
boundary gets its exact parameter t = (b - o_k) / (e_k - o_k) as a fractions.Fraction of the f32 / f64 inputs, the crossings of all axes are sorted
by (t, axis) - the stated tie rule: the lowest axis first - and the cells follow from the sorted list.

A ray is NEAR A TIE, and left out of a comparison with f64 code, when two crossings of different axes lie within `eps` in t or an end point lies
within `eps` (in units of the cell) of a cell boundary: there the f64 rounding may legitimately decide otherwise than exact arithmetic."""
import math
from fractions import Fraction

import numpy as np

SKIP_SHORT, SKIP_CULLED, SKIP_BAD = -10, -11, -12   # ALEGO_OCC_SKIP_*


def _fr(x):
    return Fraction(float(x))


def _floor(q):
    return q.numerator // q.denominator


def ray(origin, cell, n, o, e, min_range=0.0, max_range=0.0, eps=1e-9):
    """(cells (m, 3) int64, hit, near_tie) of the ray o -> e (f32 triples), or (skip code, None, False).  origin / cell: f64 triples; n: cells per axis."""
    o32, e32 = np.asarray(o, np.float32), np.asarray(e, np.float32)
    if not (np.all(np.isfinite(o32)) and np.all(np.isfinite(e32))):
        return SKIP_BAD, None, False
    O, E = [_fr(v) for v in o32], [_fr(v) for v in e32]
    org, cl = [_fr(v) for v in origin], [_fr(v) for v in cell]
    for P in (O, E):
        if any(abs((P[k] - org[k]) / cl[k]) > 2 ** 30 for k in range(3)):
            return SKIP_BAD, None, False
    len2 = sum((E[k] - O[k]) ** 2 for k in range(3))
    if len2 < _fr(min_range) ** 2:
        return SKIP_SHORT, None, False
    hit = 1
    if max_range > 0 and len2 > _fr(max_range) ** 2:
        # the one irrational step: the shortened end point is formed in f64 as the rule states it, then taken as exact
        d = [float(e32[k]) - float(o32[k]) for k in range(3)]
        f = float(max_range) / math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        E = [_fr(float(o32[k]) + d[k] * f) for k in range(3)]
        hit = 0
    q0 = [(O[k] - org[k]) / cl[k] for k in range(3)]
    q1 = [(E[k] - org[k]) / cl[k] for k in range(3)]
    c0, c1 = [_floor(q) for q in q0], [_floor(q) for q in q1]
    near = any(min(q - _floor(q), _floor(q) + 1 - q) < eps for q in q0 + q1)
    if any((c0[k] < 0 and c1[k] < 0) or (c0[k] >= n[k] and c1[k] >= n[k]) for k in range(3)):
        return SKIP_CULLED, None, near
    cross = []
    for k in range(3):
        s = (c1[k] > c0[k]) - (c1[k] < c0[k])
        for j in range(abs(c1[k] - c0[k])):
            i = c0[k] + (j + 1 if s > 0 else -j)
            cross.append(((org[k] + i * cl[k] - O[k]) / (E[k] - O[k]), k, s))
    cross.sort(key=lambda c: (c[0], c[1]))
    for a, b in zip(cross, cross[1:]):
        if a[1] != b[1] and b[0] - a[0] < eps:
            near = True
    cells, c = [list(c0)], list(c0)
    for _, k, s in cross:
        c[k] += s
        cells.append(list(c))
    assert cells[-1] == c1
    return np.array(cells, np.int64), hit, near


def generator(count=3000, seed=1):
    """the rays of the issue's generator: o ~ N(0, 5 m) in x, y and N(0, 0.3 m) in z; a normal direction with z scaled by 0.2, normalised; length
    U(0.5, 40) m; e = f32(o + dir * len).  Returns (o, e) as (count, 3) f32 and the grid (origin, cell, n)."""
    rng = np.random.default_rng(seed)
    o = (rng.standard_normal((count, 3)) * np.array([5.0, 5.0, 0.3])).astype(np.float32)
    d = rng.standard_normal((count, 3)) * np.array([1.0, 1.0, 0.2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = (o.astype(np.float64) + d * rng.uniform(0.5, 40.0, (count, 1))).astype(np.float32)
    return o, e, ((-20.0, -20.0, -2.0), (0.4, 0.4, 0.5), (100, 100, 8))


def accumulate(origin, cell, n, rays, min_range=0.0, max_range=0.0):
    """(hits, passes, stats, near) of numpy accumulation of the reference sequences; arrays (n2, n1, n0) uint32, stats as ALEGO_OCC_*"""
    hits, passes = np.zeros((n[2], n[1], n[0]), np.uint32), np.zeros((n[2], n[1], n[0]), np.uint32)
    stats, near_any = np.zeros(6, np.int64), False
    for o, e in rays:
        cells, hit, near = ray(origin, cell, n, o, e, min_range, max_range)
        near_any = near_any or near
        stats[0] += 1
        if max_range > 0 and np.all(np.isfinite(o)) and np.all(np.isfinite(e)):
            d = np.asarray(e, np.float64) - np.asarray(o, np.float64)
            L2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if not isinstance(cells, int) or cells == SKIP_CULLED:
                stats[2] += int(L2 > max_range * max_range)
        if isinstance(cells, int):
            stats[{SKIP_SHORT: 1, SKIP_CULLED: 3, SKIP_BAD: 4}[cells]] += 1
            continue
        inside = np.all((cells >= 0) & (cells < np.array(n)), axis=1)
        for m in np.nonzero(inside)[0]:
            x, y, z = cells[m]
            if m == len(cells) - 1 and hit:
                hits[z, y, x] += 1
            else:
                passes[z, y, x] += 1
        stats[5] += int(inside.sum())
    return hits, passes, stats, near_any
