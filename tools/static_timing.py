"""Kernel time of the static map (occ_mark + occ_offsets + occ_emit) on the whole archive of the 560-scan synthetic lap, next
to what the assembly costs today (map_offsets + map_gather of the same handle) and to the host twin on one core.

For every cell size of --cells a SLAM handle replays the lap with the archive on, gets occ_timing.py's grid (key poses' bounding box plus
--max-range in x and y, +/- 3 m in z, cubic cells) and integrates the archive once.  Then, for protect_radius 0 and 1, alego_map_assemble_static
(count only, leaf 0) and alego_map_assemble (count only) run --reps times after a warm-up, alternated in one process; the kernels' times come
from alego_profile_report (HIP events around each launch), the medians are kept.  alego_occ_mark_host then judges the same points once on one
core (host clock); the device verdicts must equal the twin's exactly.  Bytes: 16 read + 16 written per point by occ_mark, 1 + 16 read and 16 written
per kept point by occ_emit, plus 8 per cell read (the own cell of every point inside the grid; the neighbourhoods of the points of class 0).
One JSON line per cell size and radius; --out also writes them to a file.

    python tools/static_timing.py [--cells 0.2,0.4] [--reps 5] [--max-range 40] [--scans 560] [--out profiles/static_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alego_loader import load_package  # noqa: E402

load_package()
from alego_amd import binding, synth  # noqa: E402

ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
NEW, OLD = ("occ_mark", "occ_offsets", "occ_emit"), ("map_offsets", "map_gather")


def _timed(h, call, names):
    h.profile_enable(True)
    out = call()
    rep = h.profile_report()
    h.profile_enable(False)
    return out, {k: rep[k][0] for k in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="0.2,0.4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-range", type=float, default=40.0)
    ap.add_argument("--scans", type=int, default=560)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(a.scans)]
    L = binding.lib()
    rows = []
    for cell in [float(v) for v in a.cells.split(",")]:
        h = binding.Handle(p)
        h.map_enable(4096, 1 << 24)
        for k, pts in enumerate(scans):
            h.scan_process(pts, stages=7, stamp=0.1 * k)
        kp = h.map_keyposes()
        lo, hi = kp[:, :3].astype(np.float64).min(axis=0), kp[:, :3].astype(np.float64).max(axis=0)
        pad = np.array([a.max_range, a.max_range, 3.0])
        origin = np.floor((lo - pad) / cell) * cell
        n = np.ceil((hi + pad - origin) / cell).astype(int)
        opts = binding.occ_opts(origin, cell, n, 0.0, a.max_range)
        h.occ_enable(opts)
        h.occ_integrate()
        hits, passes = h.occ_get()
        raw = h.map_assemble(ALL)
        sz = np.concatenate([np.concatenate([kf["surf"][:, 2], kf["corner"][:, 2], kf["outlier"][:, 2]]) for kf in (h.map_get_keyframe(f) for f in range(kp.shape[0]))])
        for radius in (0, 1):
            rule = binding.static_rule(protect_radius=radius)
            new_ms, old_ms = {k: [] for k in NEW}, {k: [] for k in OLD}
            for r in range(a.reps + 1):            # (repetition 0 warms up and is dropped)
                kept, t_new = _timed(h, lambda: h._check(L.alego_map_assemble_static(h._h, 0, ALL, 0.0, binding._static_rule(rule), None, 0, None), "static"), NEW)
                _, t_old = _timed(h, lambda: h._check(L.alego_map_assemble(h._h, 0, ALL, 0.0, None, 0), "assemble"), OLD)
                if r:
                    for k in NEW:
                        new_ms[k].append(t_new[k])
                    for k in OLD:
                        old_ms[k].append(t_old[k])
            v, stats = h.occ_mark(ALL, rule)
            t0 = time.perf_counter()
            want_v, want_s = binding.occ_mark_host(opts, hits, passes, raw, rule, sz)
            host_ms = 1e3 * (time.perf_counter() - t0)
            assert np.array_equal(v, want_v) and np.array_equal(stats, want_s), "the device verdicts equal the twin's"
            assert kept == int((v != binding.STATIC_REMOVED).sum())
            med_new = {k: float(np.median(x)) for k, x in new_ms.items()}
            med_old = {k: float(np.median(x)) for k, x in old_ms.items()}
            pts_n = int(raw.shape[0])
            inside = pts_n - int(stats[binding.STATIC_OUTSIDE])
            free = int(stats[binding.STATIC_NEIGHBOUR] + stats[binding.STATIC_REMOVED])
            cell_reads = inside + free * (2 * radius + 1) ** 3      # an upper bound: a neighbourhood ends at the first occupied cell and at the grid's faces
            mark_bytes = 32 * pts_n + 8 * cell_reads
            emit_bytes = pts_n + 32 * kept
            row = dict(cell=cell, protect_radius=radius, scans=a.scans, key_frames=int(kp.shape[0]), grid=[int(x) for x in n], cells=int(np.prod(n)), points=pts_n,
                       kept=int(kept), stats=[int(x) for x in stats], reps=a.reps,
                       ms={k: [round(x, 4) for x in new_ms[k]] for k in NEW}, median_ms={k: round(med_new[k], 4) for k in NEW},
                       static_total_median_ms=round(sum(med_new.values()), 4),
                       assemble_ms={k: [round(x, 4) for x in old_ms[k]] for k in OLD}, assemble_median_ms={k: round(med_old[k], 4) for k in OLD},
                       assemble_total_median_ms=round(sum(med_old.values()), 4),
                       occ_mark_points_per_s=round(pts_n / (1e-3 * med_new["occ_mark"])), occ_mark_bytes_per_s=round(mark_bytes / (1e-3 * med_new["occ_mark"])),
                       occ_emit_bytes_per_s=round(emit_bytes / (1e-3 * med_new["occ_emit"])), cell_reads_upper_bound=int(cell_reads),
                       host_one_core_ms=round(host_ms, 2), host_points_per_s=round(pts_n / (1e-3 * host_ms)))
            rows.append(row)
            print(json.dumps(row), flush=True)
        h.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
