"""Brute-force reference of the clearance field and the cost map: every cell against every source in numpy int64, the
cap, the flags, the statistics, and the cost rule in Python scalars.  It shares no code with the library."""
import math

import numpy as np

FAR = 0xFFFFFFFF


def sources(cls, unknown_is_obstacle=False):
    cls = np.asarray(cls)
    return (cls == 100) | ((cls == -1) if unknown_is_obstacle else False)


def distance(cls, unknown_is_obstacle=False, max_cells=0):
    """(d2 uint32 of cls's shape, stats [sources, FAR cells, largest finite d2 or -1]); cls of any dimension up to 3, indexed [z, y, x]"""
    cls = np.asarray(cls, np.int8)
    shape = cls.shape
    c3 = cls.reshape((1,) * (3 - cls.ndim) + shape)
    zz, yy, xx = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in c3.shape], indexing="ij")
    cells = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], axis=1)
    src = cells[sources(c3, unknown_is_obstacle).ravel()]
    if src.shape[0] == 0:
        d2 = np.full(cells.shape[0], FAR, np.int64)
    else:
        d2 = np.full(cells.shape[0], np.iinfo(np.int64).max, np.int64)
        for a in range(0, src.shape[0], 256):   # chunks of sources bound the memory
            diff = cells[:, None, :] - src[None, a:a + 256, :]
            d2 = np.minimum(d2, (diff * diff).sum(axis=2).min(axis=1))
    if max_cells > 0:
        d2 = np.where(d2 > max_cells * max_cells, FAR, d2)
    finite = d2[d2 != FAR]
    stats = np.array([int((d2 == 0).sum()), int((d2 == FAR).sum()), int(finite.max()) if finite.size else -1], np.int64)
    return d2.astype(np.uint32).reshape(shape), stats


def cost_table(s, inscribed, radius, scaling):
    """costmap_2d's computeCost over d2 = 0 .. r r in numpy float64"""
    r = int(math.ceil(radius / s))
    dist = np.sqrt(np.arange(r * r + 1, dtype=np.float64)) * s
    table = np.where(dist <= inscribed, 253.0, np.floor(252.0 * np.exp(-scaling * (dist - inscribed))))
    table[0] = 254.0
    return table.astype(np.uint8)


def cost(cls, d2, table, unknown_is_obstacle=False, inflate_unknown=False):
    cls, d2 = np.asarray(cls), np.asarray(d2)
    out = np.zeros(cls.shape, np.uint8)
    for i in np.ndindex(*cls.shape):
        c, d = int(cls[i]), int(d2[i])
        if c == 100 or (unknown_is_obstacle and c == -1):
            out[i] = 254
            continue
        t = int(table[d]) if d != FAR and d < len(table) else 0
        if c == 0:
            out[i] = t
        else:
            out[i] = t if t >= (1 if inflate_unknown else 253) else 255
    return out
