"""Wall time of alego_map_align next to the appearance search of a slot's own archive on the same handle.

For every N of --pairs a SLAM handle of N + 1 slots replays the 560-scan synthetic lap for --steps scans from varied start scans with the
archive and the appearance descriptors on (as tools/loop_appearance_timing.py); pair i aligns slot i + 1 (source) to slot i
(destination).  The first call describes every archived frame and allocates the scratch (reported as first_call_ms); the timed calls
find nothing left to describe.  Per N, medians of --reps repetitions, host clock around the synchronous call:
  align      map_align on the N pairs with the defaults (8 queries, 2 candidates)
  appearance loop_search_appearance(verify = 1) on the same N + 1 slots
One JSON line per N.

    python tools/map_align_timing.py [--pairs 1,64,1024] [--reps 5] [--steps 251]
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

LAP = 560


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=251)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(LAP)]
    med = lambda v: round(float(np.median(v)), 4)
    for n in [int(v) for v in a.pairs.split(",")]:
        h = binding.Handle(p, n_slots=n + 1)
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, scans[k])
        for s in range(n + 1):
            h.replay_assign(s, 0, (s * 37) % LAP)
        h.map_enable(64, 1 << 18)
        h.loop_appearance_enable()
        h.batch_run(0, a.steps, stages=7 | binding.REPLAY_BAG, sync=False)
        h.synchronize()
        pairs = [(i + 1, i) for i in range(n)]
        frames = [h.map_status(s)[0] for s in range(min(n + 1, 8))]
        t0 = time.perf_counter()
        h.map_align(pairs, hyps=False)
        first = 1e3 * (time.perf_counter() - t0)
        ms_a, res = timed(lambda: h.map_align(pairs, hyps=False), a.reps)
        slots = list(range(n + 1))
        h.loop_search_appearance(slots, verify=1)
        ms_l, _ = timed(lambda: h.loop_search_appearance(slots, verify=1), a.reps)
        row = dict(pairs=n, steps=a.steps, reps=a.reps, frames_per_slot=frames, first_call_ms=round(first, 3), align_ms=[round(v, 4) for v in ms_a], align_median_ms=med(ms_a),
                   align_ms_per_pair=round(med(ms_a) / n, 5), appearance_ms=[round(v, 4) for v in ms_l], appearance_median_ms=med(ms_l),
                   appearance_ms_per_slot=round(med(ms_l) / (n + 1), 5), aligned=sum(r["status"] == 2 for r in res), attempted=sum(r["status"] >= 1 for r in res),
                   accepted_hypotheses=sum(r["n_accepted"] for r in res))
        h.profile_enable(True)
        h.map_align(pairs, hyps=False)
        rep = h.profile_report()
        h.profile_enable(False)
        row["kernels_ms"] = {k: round(v[0], 4) for k, v in rep.items() if k.startswith(("rl_", "ma_", "lc_", "vox"))}
        h.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
