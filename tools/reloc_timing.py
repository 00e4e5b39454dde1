"""Wall time of alego_loc_relocalize against the host twins' brute force.

The 560-scan synthetic lap is mapped once; its key frames are the 50-frame map.  The synthetic large map repeats them --big-frames times
over: copy j keeps every point with probability 0.8, is rotated about z by a random angle (its key pose turned back by the same angle, so
it still describes the same place) and moved 200 m along y per block of copies.  For every N of --slots a localising handle of N slots
replays two scans per slot from varied start scans, so that every slot has had its first mapping frame and nothing else; then, per map:
  search     loc_relocalize(verify = 0), --reps repetitions, host clock around the synchronous call
  total      loc_relocalize(verify = 1, apply = 0); verification = total - search
  pruned     share of (slot, frame) pairs the ring-key bound kept from the second round ("rl_stats")
  rl_search  its HIP-event time (alego_profile_report) over one call with the bound and one with ALEGO_RL_BRUTE = 1
  host       alego_reloc_match over all frames for --host-queries of the slots' descriptors on one core, per query
One JSON line per (map, N).

    python tools/reloc_timing.py [--slots 1,64,1024] [--reps 5] [--big-frames 8192] [--host-queries 2]
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
MAX_RANGE, Z_OFFSET = 40.0, 4.0


def big_map(frames, n, rng):
    out = []
    for j in range(n):
        f = frames[j % len(frames)]
        a = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(a), np.sin(a)
        pose = np.array(f[0], np.float32).copy()
        pose[1] += 200.0 * (j // len(frames))
        pose[5] -= a   # (roll and pitch of the lap's key poses are ~1e-3: the rotated cloud under the turned pose is the same place to that order)
        clouds = []
        for cl in f[1:]:
            cl = cl[rng.random(len(cl)) < 0.8]
            xy = cl[:, :2].astype(np.float64) @ np.array([[c, -s], [s, c]]).T
            clouds.append(np.c_[xy, cl[:, 2:]].astype(np.float32))
        out.append((pose,) + tuple(clouds))
    return out


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
    ap.add_argument("--big-frames", type=int, default=8192)
    ap.add_argument("--host-queries", type=int, default=2)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    scans = [synth.scan(p, k) for k in range(LAP)]
    hm = binding.Handle(p)
    hm.map_enable(256, 1 << 20)
    for k in range(LAP):
        hm.scan_process(scans[k], stages=7)
    frames = [hm.map_get_keyframe(i) for i in range(hm.map_status()[0])]
    hm.close()
    lap = [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames]
    maps = [("lap", lap)]
    if a.big_frames > 0:
        maps.append(("synthetic", big_map(lap, a.big_frames, np.random.default_rng(1))))
    med = lambda v: round(float(np.median(v)), 4)
    for name, fr in maps:
        mdesc = None
        for n in [int(v) for v in a.slots.split(",")]:
            row = dict(map=name, map_frames=len(fr), slots=n, reps=a.reps)
            h = binding.Handle(p, n_slots=n)
            h.replay_create(1, LAP)
            for k in range(LAP):
                h.replay_load(0, k, scans[k])
            t0 = time.perf_counter()
            h.loc_enable(fr, 0.0)
            row["loc_enable_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            h.reloc_enable(MAX_RANGE, Z_OFFSET)
            row["reloc_enable_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            for s in range(n):
                h.replay_assign(s, 0, (s * 37) % LAP)
            h.batch_run(0, 2, stages=7 | binding.REPLAY_BAG, sync=True)
            slots = list(range(n))
            h.loc_relocalize(slots, verify=1)   # warm-up: scratch is allocated by the first call
            ms_s, _ = timed(lambda: h.loc_relocalize(slots, verify=0), a.reps)
            ev, total = h.debug_get("rl_stats")
            ms_t, res = timed(lambda: h.loc_relocalize(slots, verify=1), a.reps)
            row.update(search_ms=[round(v, 4) for v in ms_s], search_median_ms=med(ms_s), total_ms=[round(v, 4) for v in ms_t], total_median_ms=med(ms_t),
                       verify_median_ms=round(med(ms_t) - med(ms_s), 4), search_ms_per_slot=round(med(ms_s) / n, 5), total_ms_per_slot=round(med(ms_t) / n, 5),
                       pairs_evaluated=int(ev), pairs=int(total), pruned_share=round(1.0 - ev / max(total, 1), 4),
                       accepted=sum(r["status"] == 2 for r in res))
            for tag, brute in (("pruned", 0), ("brute", 1)):
                h.set_option("ALEGO_RL_BRUTE", brute)
                h.profile_enable(True)
                h.loc_relocalize(slots, verify=0)
                rep = h.profile_report()
                h.profile_enable(False)
                row[f"rl_search_{tag}_ms"] = round(rep.get("rl_search", (0.0, 0))[0], 4)
                row[f"search_kernels_{tag}_ms"] = {k: round(v[0], 4) for k, v in rep.items() if k.startswith("rl_")}
            h.set_option("ALEGO_RL_BRUTE", 0)
            if mdesc is None:
                mdesc = h.debug_get("rl_map_desc", cap_bytes=len(fr) * 1200 + 16).reshape(-1, 1200)
            nq = min(a.host_queries, n)
            t0 = time.perf_counter()
            for s in range(nq):
                q = h.debug_get("rl_query_desc", slot=s)
                best = min((binding.reloc_match(q, m) + (i,) for i, m in enumerate(mdesc)), key=lambda t: (t[0], t[2]))
                assert best[2] == res[s]["cand_id"][0] and best[0] == res[s]["cand_dist"][0] and best[1] == res[s]["cand_shift"][0], (s, best, res[s])
            row["host_brute_ms_per_query"] = round(1e3 * (time.perf_counter() - t0) / nq, 3)
            row["host_over_device_per_slot"] = round(row["host_brute_ms_per_query"] / max(row["search_ms_per_slot"], 1e-9), 1)
            h.close()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
