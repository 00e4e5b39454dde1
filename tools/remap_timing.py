"""What solution remapping (alego_remap_enable) costs at the benchmark's shape, mode on against mode off in one process.

Two handles are set up the way bench.py sets up its timed handle (geometry 16x1800, key-frame capacities 8192 / 2048, --bags recorded laps shared
by --streams slots, start scans spread over the lap, --prime untimed scans to fill the local maps); one of them calls alego_remap_enable before
its first scan.  Both then run --steps scans between host clocks, alternating --reps times (A B A B: a drift of the box hits both), and once more
with the library's own profiler (alego_profile_enable / alego_profile_report: HIP events around every launch), which gives lm_solve_remap's time
per launch next to lm_solve's in the same run.  With the mode off the profiler's kernel list must not hold a _remap kernel: the tool asserts it.
Then one stream alone, on and off: the solver's time where nothing else shares the chip (the Jacobi tail is a serial chain on one wavefront while
the other three of the workgroup wait).  The poses of the two handles differ by design; the tool reports how many records hold a direction.

One JSON line.

    python tools/remap_timing.py [--streams 2048] [--bags 8] [--prime 560] [--steps 20] [--reps 3] [--eig-min 100]
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


def _solver(kern):
    """(kernel name, ms, launches) of the solver kernel a profile holds"""
    for name in ("lm_solve_remap", "lm_solve"):
        if name in kern:
            return (name,) + tuple(kern[name])
    return ("-", 0.0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--prime", type=int, default=LAP)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eig-min", type=float, default=0.0)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    p.kf_cap_surf, p.kf_cap_outlier = 8192, 2048
    with ThreadPoolExecutor(max_workers=8) as ex:   # (the generator releases the GIL)
        flat = list(ex.map(lambda bk: synth.scan(p, bk[1], stream=bk[0]), [(b, k) for b in range(a.bags) for k in range(LAP)]))
    bags = [flat[b * LAP:(b + 1) * LAP] for b in range(a.bags)]
    stages = 7 | binding.REPLAY_BAG

    def make(n_streams, on):
        h = binding.Handle(p, n_slots=n_streams, ring_len=1)
        h.replay_create(a.bags, LAP)
        for b, bag in enumerate(bags):
            for k, s in enumerate(bag):
                h.replay_load(b, k, s)
        for s in range(n_streams):
            h.replay_assign(s, s % a.bags, ((s // a.bags) * 37) % LAP)
        if on:
            h.remap_enable(binding.remap_opts(a.eig_min))
        h.batch_run(0, a.prime, stages)
        return h

    def profile(h, step):
        h.profile_enable(True)
        h.batch_run(step, a.steps, stages)
        kern = h.profile_report()
        h.profile_enable(False)
        return kern

    hs = {name: make(a.streams, name == "on") for name in ("off", "on")}
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
    kern = {name: profile(hs[name], step) for name in ("off", "on")}
    assert not any("_remap" in k for k in kern["off"]), sorted(kern["off"])      # nothing of the mode is launched without the enabling call
    assert "lm_solve_remap" in kern["on"] and "lm_solve" not in kern["on"], sorted(kern["on"])
    recs = hs["on"].remap_get(list(range(min(a.streams, 256))))
    groups, per_launch = hs["on"].stream_groups()
    for h in hs.values():
        h.close()
    one = {}
    for name in ("off", "on"):   # one stream alone
        h = make(1, name == "on")
        one[name] = _solver(profile(h, a.prime))
        h.close()
    med = lambda v: float(np.median(v))
    on_name, on_ms, on_n = _solver(kern["on"])
    off_name, off_ms, off_n = _solver(kern["off"])
    frames_per_slot = a.steps / p.lm_every   # mapping frames of a slot in the profiled steps
    good = [r for r in recs if r["status"] == 1]
    row = dict(streams=a.streams, bags=a.bags, prime=a.prime, steps=a.steps, reps=a.reps, eig_min=a.eig_min or 100.0, stream_groups=groups, slots_per_launch=per_launch,
               scans_per_s_off=[round(v) for v in rate["off"]], scans_per_s_on=[round(v) for v in rate["on"]],
               median_off=round(med(rate["off"])), median_on=round(med(rate["on"])), on_over_off=round(med(rate["on"]) / med(rate["off"]), 4),
               remap_kernels_launched_off=False, solver_kernel_on=on_name, solver_kernel_off=off_name, solver_launches_on=on_n, solver_launches_off=off_n,
               lm_solve_remap_us_per_launch=round(1e3 * on_ms / max(on_n, 1), 2), lm_solve_us_per_launch=round(1e3 * off_ms / max(off_n, 1), 2),
               lm_solve_remap_us_per_frame_and_slot=round(1e3 * on_ms / (frames_per_slot * a.streams), 4),
               lm_solve_us_per_frame_and_slot=round(1e3 * off_ms / (frames_per_slot * a.streams), 4),
               remap_over_plain=round(on_ms / off_ms, 4) if off_ms else None,
               one_stream_lm_solve_remap_us_per_launch=round(1e3 * one["on"][1] / max(one["on"][2], 1), 2),
               one_stream_lm_solve_us_per_launch=round(1e3 * one["off"][1] / max(one["off"][2], 1), 2),
               records_status_1=len(good), records_read=len(recs), n_held_hist=np.bincount([r["n_held"] for r in good], minlength=7).tolist())
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
