"""Wall time of alego_loop_search_appearance against its two baselines on the same archive: the radius search
alego_loop_search and the host twin alego_loop_appearance_candidates on one core.

For every N of --slots a SLAM handle of N slots replays the 560-scan synthetic lap for --steps scans from varied start scans with the
archive on (as tests/test_loop_search.py::replay_handle); the first appearance search describes every archived frame (reported as
first_call_ms), the timed calls find nothing left to describe.  Per N, medians of --reps repetitions, host clock around the synchronous call:
  search     loop_search_appearance(verify = 0)
  total      loop_search_appearance(verify = 1); verification = total - search
  radius     loop_search on the same handle
  host       loop_appearance_candidates on the descriptors, key poses and stamps of --host-queries of the slots, per slot
One JSON line per N.

    python tools/loop_appearance_timing.py [--slots 1,64,1024] [--reps 5] [--steps 545] [--host-queries 2]
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
    ap.add_argument("--slots", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=545)
    ap.add_argument("--host-queries", type=int, default=2)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(LAP)]
    med = lambda v: round(float(np.median(v)), 4)
    for n in [int(v) for v in a.slots.split(",")]:
        h = binding.Handle(p, n_slots=n)
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, scans[k])
        for s in range(n):
            h.replay_assign(s, 0, (s * 37) % LAP)
        h.map_enable(128, 1 << 19)
        h.loop_appearance_enable()
        h.batch_run(0, a.steps, stages=7 | binding.REPLAY_BAG, sync=False)
        h.synchronize()
        slots = list(range(n))
        frames = [h.map_status(s)[0] for s in range(min(n, 8))]
        t0 = time.perf_counter()
        h.loop_search_appearance(slots, verify=1)   # describes every frame; allocates the search and ICP scratch
        first = 1e3 * (time.perf_counter() - t0)
        ms_s, _ = timed(lambda: h.loop_search_appearance(slots, verify=0), a.reps)
        ev, total = h.debug_get("rl_stats")
        ms_t, res = timed(lambda: h.loop_search_appearance(slots, verify=1), a.reps)
        h.loop_search(slots)
        ms_r, rad = timed(lambda: h.loop_search(slots), a.reps)
        row = dict(slots=n, steps=a.steps, reps=a.reps, frames_per_slot=frames, first_call_ms=round(first, 3),
                   search_ms=[round(v, 4) for v in ms_s], search_median_ms=med(ms_s), total_ms=[round(v, 4) for v in ms_t], total_median_ms=med(ms_t),
                   verify_median_ms=round(med(ms_t) - med(ms_s), 4), search_ms_per_slot=round(med(ms_s) / n, 5), total_ms_per_slot=round(med(ms_t) / n, 5),
                   radius_ms=[round(v, 4) for v in ms_r], radius_median_ms=med(ms_r), radius_ms_per_slot=round(med(ms_r) / n, 5),
                   pairs_evaluated=int(ev), pairs=int(total), accepted=sum(r["status"] == 2 for r in res), attempted=sum(r["status"] >= 1 for r in res),
                   radius_accepted=sum(r["status"] == 2 for r in rad), radius_attempted=sum(r["status"] >= 1 for r in rad))
        h.profile_enable(True)
        h.loop_search_appearance(slots, verify=0)
        rep = h.profile_report()
        h.profile_enable(False)
        row["search_kernels_ms"] = {k: round(v[0], 4) for k, v in rep.items() if k.startswith(("rl_", "la_"))}
        nq = min(a.host_queries, n)
        host = []
        for s in range(nq):
            nf = h.map_status(s)[0]
            desc = h.debug_get("la_desc", slot=s).reshape(-1, 1200)
            kp = np.array([h.map_get_keyframe(j, slot=s)["pose"] for j in range(nf)], np.float32)
            st = h.map_get_stamps(slot=s)
            ms_h, got = timed(lambda: binding.loop_appearance_candidates(desc, kp, st, p.lc_min_time_gap), a.reps)
            assert np.array_equal(got[0], res[s]["cand_id"]) and np.array_equal(got[1], res[s]["cand_dist"]) and np.array_equal(got[2], res[s]["cand_shift"]), (s, got, res[s])
            host.append(med(ms_h))
        row["host_twin_ms_per_slot"] = med(host)
        row["host_over_device_per_slot"] = round(row["host_twin_ms_per_slot"] / max(row["search_ms_per_slot"], 1e-9), 1)
        h.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
