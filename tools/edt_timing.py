"""Kernel times of the clearance field on the grids of the 560-scan synthetic lap, next to the host twin on one core.

For every cell size of --cells a SLAM handle replays the lap with the archive on, gets section 24's 3-D grid (the key poses' bounding box plus
--max-range in x and y and +/- 3 m in z, cubic cells) and integrates the archive once.  alego_occ_distance then runs --reps + 1 times on the 3-D grid
and on its collapsed 2-D form (the first is a warm-up and is dropped): the kernels' times come from alego_profile_report (HIP events around each
launch), the whole call including the copy of d2 from the host clock; medians are kept.  alego_occ_distance_host gives the CPU reference on one core
and the check that device and twin agree at that size.  Bytes per second are made from the bytes a pass has to move (pass X: a class read and a
u32 written per cell; passes Y and Z: a u32 read and one written; the end: a u32 read), not from what the envelopes' stacks add to that.
alego_occ_costmap is timed the same way on the collapsed grid.
One JSON line per grid; --out also writes them to a file.

    python tools/edt_timing.py [--cells 0.2,0.4] [--reps 5] [--max-range 40] [--scans 560] [--out profiles/edt_timing.json]
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

KERNELS = ("occ_classify", "edt_pass_x", "edt_pass_y", "edt_pass_z", "edt_finish")
MUST_MOVE = dict(occ_classify=None, edt_pass_x=5, edt_pass_y=8, edt_pass_z=8, edt_finish=4)   # bytes per cell (occ_classify reads the counts of every layer)
HBM_PEAK, HBM_MEASURED = 8.0e12, 6.29e12   # bytes per second: the specification and a float4 copy


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
        h.occ_enable(binding.occ_opts(origin, cell, n, 0.0, a.max_range))
        h.occ_integrate()
        infl = binding.occ_inflation(0.35, 2.0, 3.0)
        for collapse in (False, True):
            dom = [int(n[0]), int(n[1]), 1 if collapse else int(n[2])]
            cells = int(np.prod(dom))
            ms = {k: [] for k in KERNELS}
            call_ms, cost_ms, cost_call_ms = [], [], []
            for r in range(a.reps + 1):            # (repetition 0 warms up and is dropped)
                h.profile_enable(True)
                t0 = time.perf_counter()
                d2, stats = h.occ_distance(collapse_z=collapse)
                t = 1e3 * (time.perf_counter() - t0)
                rep = h.profile_report()
                h.profile_enable(False)
                if r:
                    call_ms.append(t)
                    for k in KERNELS:
                        ms[k].append(rep[k][0] if k in rep else 0.0)
                if collapse:
                    h.profile_enable(True)
                    t0 = time.perf_counter()
                    h.occ_costmap(infl, collapse_z=True)
                    t = 1e3 * (time.perf_counter() - t0)
                    rep = h.profile_report()
                    h.profile_enable(False)
                    if r:
                        cost_call_ms.append(t); cost_ms.append(rep["edt_cost_k"][0])
            cls = h.occ_classify(collapse_z=collapse)
            t0 = time.perf_counter()
            want, ws = binding.occ_distance_host(cls)
            host_ms = 1e3 * (time.perf_counter() - t0)
            agree = bool(np.array_equal(d2, want) and stats.tolist() == ws.tolist())
            assert agree, "the device's d2 and statistics equal the twin's"
            med = {k: float(np.median(v)) for k, v in ms.items()}
            edt_ms = sum(med[k] for k in KERNELS if k != "occ_classify")
            passes = {}
            for k in KERNELS:
                row = dict(ms=[round(v, 4) for v in ms[k]], median_ms=round(med[k], 4))
                if med[k] > 0:
                    row["cells_per_s"] = round(cells / (1e-3 * med[k]))
                    if MUST_MOVE[k]:
                        bps = MUST_MOVE[k] * cells / (1e-3 * med[k])
                        row.update(bytes_per_cell=MUST_MOVE[k], bytes_per_s=round(bps), of_hbm_peak=round(bps / HBM_PEAK, 4), of_hbm_measured=round(bps / HBM_MEASURED, 4))
                passes[k] = row
            lines = dict(edt_pass_x=dom[1] * dom[2], edt_pass_y=dom[0] * dom[2] if dom[1] > 1 else 0, edt_pass_z=dom[0] * dom[1] if dom[2] > 1 else 0)
            row = dict(cell=cell, collapsed=collapse, scans=a.scans, key_frames=int(kp.shape[0]), grid=dom, cells=cells, sources=int(stats[0]), far_cells=int(stats[1]),
                       max_d2=int(stats[2]), reps=a.reps, lines_per_pass=lines, kernels=passes, transform_kernels_median_ms=round(edt_ms, 4),
                       transform_cells_per_s=round(cells / (1e-3 * edt_ms)), call_with_copy_ms=[round(v, 3) for v in call_ms],
                       call_with_copy_median_ms=round(float(np.median(call_ms)), 3), host_one_core_ms=round(host_ms, 1),
                       host_cells_per_s=round(cells / (1e-3 * host_ms)), device_equals_twin=agree)
            if collapse:
                row.update(costmap_kernel_median_ms=round(float(np.median(cost_ms)), 4), costmap_call_median_ms=round(float(np.median(cost_call_ms)), 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        h.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
