"""Kernel time of occ_cast on the whole archive of the 560-scan synthetic lap, next to the host twin on one core.

For every cell size of --cells a SLAM handle replays the lap with the archive on, then gets a 3-D grid over the key poses' bounding box plus
--max-range in x and y and +/- 3 m in z (cubic cells).  For every piece length of --pieces (0: one lane per ray, the baseline) the archive is
integrated --reps times after a clear; occ_cast's time comes from alego_profile_report (HIP events around the launch), the median is kept.
All piece lengths run in the same process on the same handle, alternated rep by rep.  The same rays then go through alego_occ_integrate_host
once on one core (host clock): the CPU reference a speed figure is made against.  The device counts must equal the twin's exactly.
One JSON line per cell size; --out also writes them to a file.  --dry: for a library built with -DALEGO_OCC_DRY_RUN (ALEGO_LIB names it), whose
occ_cast walks without adding: the difference to the normal build is what the adds cost.

    python tools/occ_timing.py [--cells 0.2,0.4] [--pieces 0,8,16,32,64,128] [--reps 5] [--max-range 40] [--scans 560] [--out profiles/occ_timing.json] [--dry]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="0.2,0.4")
    ap.add_argument("--pieces", default="0,8,16,32,64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-range", type=float, default=40.0)
    ap.add_argument("--scans", type=int, default=560)
    ap.add_argument("--out", default="")
    ap.add_argument("--dry", action="store_true", help="the library is a -DALEGO_OCC_DRY_RUN build (ALEGO_LIB): its counts are not compared")
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(a.scans)]
    pieces = [int(v) for v in a.pieces.split(",")]
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
        ms = {pc: [] for pc in pieces}
        stats = None
        for r in range(a.reps + 1):            # (repetition 0 warms up and is dropped)
            for pc in pieces:
                h.debug_occ_piece(pc)
                h.occ_clear()
                h.profile_enable(True)
                stats = h.occ_integrate()
                t = h.profile_report()["occ_cast"][0]
                h.profile_enable(False)
                if r:
                    ms[pc].append(t)
        hits, passes = h.occ_get()
        pts = h.map_assemble(ALL | binding.MAP_FRAME_ID)
        t0 = time.perf_counter()
        want = binding.occ_integrate_host(opts, kp, pts)
        host_ms = 1e3 * (time.perf_counter() - t0)
        assert a.dry or np.array_equal(hits, want[0]) and np.array_equal(passes, want[1]) and np.array_equal(stats, want[2]), "the device counts equal the twin's"
        med = {pc: float(np.median(v)) for pc, v in ms.items()}
        upd = int(stats[binding.OCC_UPDATES])
        row = dict(dry_run=bool(a.dry), cell=cell, scans=a.scans, key_frames=int(kp.shape[0]), grid=[int(v) for v in n], cells=int(np.prod(n)), max_range=a.max_range,
                   rays=int(stats[binding.OCC_RAYS]), truncated=int(stats[binding.OCC_TRUNCATED]), culled=int(stats[binding.OCC_CULLED]), updates=upd,
                   updates_per_ray=round(upd / max(1, int(stats[binding.OCC_RAYS])), 1), reps=a.reps,
                   occ_cast_ms={str(pc): [round(v, 4) for v in ms[pc]] for pc in pieces},
                   occ_cast_median_ms={str(pc): round(med[pc], 4) for pc in pieces},
                   updates_per_s={str(pc): round(upd / (1e-3 * med[pc])) for pc in pieces},
                   host_one_core_ms=round(host_ms, 1), host_updates_per_s=round(upd / (1e-3 * host_ms)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        h.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
