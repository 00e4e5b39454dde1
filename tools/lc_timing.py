"""Wall time of the batched loop-closure search (alego_loop_search) against one alego_loop_closure_icp per slot on
the same frames.

A handle of max(--slots) slots replays the 560-scan synthetic lap from varied start scans for --steps scans with the key-frame archive
on; then alego_loop_search is timed over the first N slots for every N of --slots.  Both calls are synchronous, so host wall time is
device-synchronised time.  The single-attempt path is timed on the first --single slots that have a candidate, with their frames read
from the archive beforehand (not timed).  Every figure is a median over --reps calls.

    python tools/lc_timing.py [--slots 1,64,256,1024] [--steps 420] [--reps 5] [--single 32]
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


def median_s(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64,256,1024")
    ap.add_argument("--steps", type=int, default=420)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", type=int, default=32)
    a = ap.parse_args()
    sizes = [int(v) for v in a.slots.split(",")]
    p = synth.default_params(16, 1800)
    n = max(sizes)
    h = binding.Handle(p, n_slots=n)
    h.replay_create(1, LAP)
    for k in range(LAP):
        h.replay_load(0, k, synth.scan(p, k))
    for s in range(n):
        h.replay_assign(s, 0, (s * 37) % LAP)
    h.map_enable(256, 1 << 19)
    h.batch_run(0, a.steps, stages=7 | binding.REPLAY_BAG, sync=True)
    rows = []
    res = h.loop_search(list(range(n)))
    for N in sizes:
        sl = list(range(N))
        t = median_s(lambda: h.loop_search(sl), a.reps)
        att = sum(1 for r in res[:N] if r["status"] > 0)
        rows.append(dict(slots=N, attempts=att, batched_ms=1e3 * t, batched_ms_per_slot=1e3 * t / N))
    # one alego_loop_closure_icp per slot on the same frames
    frames_of = []
    for s in range(n):
        r = res[s]
        if r["status"] <= 0:
            continue
        lo, hi = max(0, r["closest_id"] - p.lc_search_num), min(r["latest_id"] - 1, r["closest_id"] + p.lc_search_num)
        fr = []
        for j in [r["latest_id"]] + list(range(lo, hi + 1)):
            k = h.map_get_keyframe(j, slot=s)
            fr.append((k["pose"], k["corner"], k["surf"], k["outlier"]))
        frames_of.append(fr)
        if len(frames_of) >= a.single:
            break
    per = []
    for fr in frames_of:
        per.append(median_s(lambda: h.loop_closure_icp(fr), a.reps))
    single_ms = 1e3 * float(np.median(per)) if per else float("nan")
    h.close()
    print("| slots | attempts | alego_loop_search (ms) | per slot (ms) | one alego_loop_closure_icp per slot (ms per slot) |")
    print("|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['slots']} | {r['attempts']} | {r['batched_ms']:.2f} | {r['batched_ms_per_slot']:.3f} | {single_ms:.2f} |")
    print(json.dumps(dict(rows=rows, single_ms_per_slot=single_ms, single_slots_timed=len(per), steps=a.steps, reps=a.reps)))


if __name__ == "__main__":
    main()
