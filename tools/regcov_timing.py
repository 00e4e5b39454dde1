"""What lm_regcov costs per mapping frame and slot at the benchmark's shape, feature on against feature off in one process.

Two handles are set up the way bench.py sets up its timed handle (geometry 16x1800, key-frame capacities 8192 / 2048, --bags recorded laps shared
by --streams slots, start scans spread over the lap, --prime untimed scans to fill the local maps); one of them calls alego_regcov_enable before
its first scan.  Both then run --steps scans between host clocks, alternating --reps times (A B A B: a drift of the box hits both), and once more
with the library's own profiler (alego_profile_enable / alego_profile_report: HIP events around every launch), which gives the kernel's time next
to lm_solve's in the same run.  The poses of the two handles are compared at the end: the feature changes nothing it does not own.

One JSON line: scans/s of either handle, the difference, lm_regcov's and lm_solve's microseconds per launch and per mapping frame and slot.

    python tools/regcov_timing.py [--streams 4096] [--bags 8] [--prime 560] [--steps 20] [--reps 3]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alego_loader import load_package  # noqa: E402

load_package()
from alego_amd import binding, synth  # noqa: E402

LAP = 560


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--prime", type=int, default=LAP)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    p.kf_cap_surf, p.kf_cap_outlier = 8192, 2048
    with ThreadPoolExecutor(max_workers=8) as ex:   # (the generator releases the GIL)
        flat = list(ex.map(lambda bk: synth.scan(p, bk[1], stream=bk[0]), [(b, k) for b in range(a.bags) for k in range(LAP)]))
    bags = [flat[b * LAP:(b + 1) * LAP] for b in range(a.bags)]
    stages = 7 | binding.REPLAY_BAG
    hs = {}
    for name in ("off", "on"):
        h = binding.Handle(p, n_slots=a.streams, ring_len=1)
        h.replay_create(a.bags, LAP)
        for b, bag in enumerate(bags):
            for k, s in enumerate(bag):
                h.replay_load(b, k, s)
        for s in range(a.streams):
            h.replay_assign(s, s % a.bags, ((s // a.bags) * 37) % LAP)
        if name == "on":
            h.regcov_enable()
        h.batch_run(0, a.prime, stages)
        hs[name] = h
    step = a.prime
    rate = {"off": [], "on": []}
    for _ in range(a.reps):
        for name in ("off", "on"):
            h = hs[name]
            h.synchronize()
            t0 = time.perf_counter()
            h.batch_run(step, a.steps, stages, sync=False)
            h.synchronize()
            rate[name].append(a.streams * a.steps / (time.perf_counter() - t0))
        step += a.steps
    kern = {}
    for name in ("off", "on"):
        h = hs[name]
        h.profile_enable(True)
        h.batch_run(step, a.steps, stages)
        kern[name] = h.profile_report()
        h.profile_enable(False)
    step += a.steps
    same = all(np.array_equal(np.r_[hs["off"].batch_get_pose(s)[2]["t"], hs["off"].batch_get_pose(s)[2]["q"]],
                              np.r_[hs["on"].batch_get_pose(s)[2]["t"], hs["on"].batch_get_pose(s)[2]["q"]]) for s in range(0, a.streams, max(1, a.streams // 64)))
    recs = hs["on"].regcov_get(list(range(min(a.streams, 256))))
    groups, per_launch = hs["on"].stream_groups()
    med = lambda v: float(np.median(v))
    rc_ms, rc_n = kern["on"].get("lm_regcov", (0.0, 0))
    so_ms, so_n = kern["on"].get("lm_solve", (0.0, 0))
    so0_ms, so0_n = kern["off"].get("lm_solve", (0.0, 0))
    frames_per_slot = a.steps / p.lm_every   # mapping frames of a slot in the profiled steps
    row = dict(streams=a.streams, bags=a.bags, prime=a.prime, steps=a.steps, reps=a.reps, stream_groups=groups, slots_per_launch=per_launch,
               scans_per_s_off=[round(v) for v in rate["off"]], scans_per_s_on=[round(v) for v in rate["on"]],
               median_off=round(med(rate["off"])), median_on=round(med(rate["on"])), on_over_off=round(med(rate["on"]) / med(rate["off"]), 4),
               lm_regcov_launched_off="lm_regcov" in kern["off"], lm_regcov_launches=rc_n, lm_regcov_us_per_launch=round(1e3 * rc_ms / max(rc_n, 1), 2),
               lm_solve_us_per_launch=round(1e3 * so_ms / max(so_n, 1), 2), lm_solve_us_per_launch_off=round(1e3 * so0_ms / max(so0_n, 1), 2),
               lm_regcov_us_per_frame_and_slot=round(1e3 * rc_ms / (frames_per_slot * a.streams), 4),
               lm_solve_us_per_frame_and_slot=round(1e3 * so_ms / (frames_per_slot * a.streams), 4),
               lm_regcov_over_lm_solve=round(rc_ms / so_ms, 4) if so_ms else None,
               poses_bit_equal=bool(same), records_status_1=sum(r["status"] == 1 for r in recs), records_read=len(recs),
               n_degenerate_hist=np.bincount([r["n_degenerate"] for r in recs if r["status"] == 1], minlength=7).tolist())
    for h in hs.values():
        h.close()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
