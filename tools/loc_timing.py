"""Wall time per step of localisation mode (alego_loc_enable) against SLAM mode of the same build.

The 560-scan synthetic lap is mapped once on a one-slot handle with the key-frame archive on; its key frames are the map.  Then, for every
N of --slots, two handles of N slots replay the lap from the bag store from varied start scans:
  loc   alego_loc_enable on the map; every slot is placed at the mapping run's pose of its start scan (alego_lm_apply_correction +
        alego_set_lm_params);
  slam  plain SLAM, primed with one lap so that its windows are full (as bench.py primes).
Both are timed alternately in one process: a host clock around alego_batch_run(sync = 0) + alego_synchronize, --warmup steps, then --reps
repetitions of --steps steps each (the handles keep running from where they are).  Two shapes: the defaults (K = 50, radius 50: the window is
the whole 50-frame map and never changes) and K = 10, radius 6 (windows change; rebuilds per slot and step are reported).  One more
localisation run of the first shape is profiled (alego_profile_report).  One JSON line per (shape, N); a size whose handles do not fit the
device is reported as such.

    python tools/loc_timing.py [--slots 1024,4096] [--steps 200] [--warmup 20] [--reps 5] [--kf-cap 8192]
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


def quat_R(q):
    w, x, y, z = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def params(a, k):
    p = synth.default_params(16, 1800)
    if a.kf_cap > 0:
        p.kf_cap_surf, p.kf_cap_outlier = a.kf_cap, max(256, a.kf_cap // 4)
    if k:
        p.recent_keyframe_num = k
    return p


def timed(h, first, steps):
    t0 = time.perf_counter()
    h.batch_run(first, steps, stages=7 | binding.REPLAY_BAG, sync=False)
    h.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1024")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kf-cap", type=int, default=8192, help="alego_params.kf_cap_surf (outliers a quarter), as bench.py sets it for 16 x 1800")
    a = ap.parse_args()
    scans = [synth.scan(params(a, 0), k) for k in range(LAP)]
    hm = binding.Handle(params(a, 0))
    hm.map_enable(256, 1 << 20)
    track = np.zeros((LAP, 7))
    for k in range(LAP):
        _, _, mp = hm.scan_process(scans[k], stages=7)
        track[k] = np.r_[mp["t"], mp["q"]]
    frames = [hm.map_get_keyframe(i) for i in range(hm.map_status()[0])]
    hm.close()
    fr = [(f["pose"], f["corner"], f["surf"], f["outlier"]) for f in frames]
    start = lambda s: (s * 37) % LAP

    def handle(p, n, loc, radius):
        h = binding.Handle(p, n_slots=n)
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, scans[k])
        if loc:
            h.loc_enable(fr, radius)
        for s in range(n):
            h.replay_assign(s, 0, start(s))
            if loc:
                t, q = track[start(s), :3], track[start(s), 3:]
                R = quat_R(q)
                h.lm_apply_correction(np.c_[R, t].reshape(12), slot=s)
                h.set_lm_params(np.r_[t, np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[2, 1], R[2, 2])), np.arctan2(R[1, 0], R[0, 0])], slot=s)
        return h

    for n in [int(v) for v in a.slots.split(",")]:
        for shape, (K, radius) in (("default", (0, 0.0)), ("K10_r6", (10, 6.0))):
            p = params(a, K)
            row = dict(shape=shape, K=p.recent_keyframe_num, radius=radius or 50.0, slots=n, map_frames=len(fr), steps=a.steps, warmup=a.warmup)
            try:
                hl = handle(p, n, True, radius)
                hs = handle(p, n, False, 0.0)
            except binding.AlegoError as e:
                row.update(fits=False, error=str(e))
                print(json.dumps(row), flush=True)
                continue
            row["fits"] = True
            hs.batch_run(0, LAP, stages=7 | binding.REPLAY_BAG, sync=True)   # prime: one lap fills the windows
            pos = {id(hl): 0, id(hs): LAP}
            for h in (hl, hs):
                timed(h, pos[id(h)], a.warmup)
                pos[id(h)] += a.warmup
            reb0 = sum(hl.loc_status(s)["rebuilds"] for s in range(n))
            ms = {"loc": [], "slam": []}
            for _ in range(a.reps):
                for name, h in (("loc", hl), ("slam", hs)):
                    ms[name].append(timed(h, pos[id(h)], a.steps))
                    pos[id(h)] += a.steps
            reb = sum(hl.loc_status(s)["rebuilds"] for s in range(n)) - reb0
            st = [hl.loc_status(s) for s in range(0, n, max(1, n // 64))]
            for name in ms:
                row[name + "_ms_per_step"] = [round(v, 4) for v in ms[name]]
                row[name + "_median"] = round(float(np.median(ms[name])), 4)
                row[name + "_spread"] = round(float(max(ms[name]) - min(ms[name])), 4)
            row["loc_rebuilds_per_slot_step"] = round(reb / (n * a.reps * a.steps), 5)
            row["loc_window_mean"] = round(float(np.mean([s["window"] for s in st])), 2)
            row["loc_optimized_share"] = round(float(np.mean([s["optimized"] for s in st])), 3)
            bad = 0
            for s in range(n):
                try:
                    hl.batch_get_pose(s)
                except binding.AlegoError:
                    bad += 1
            row["loc_slots_with_errors"] = bad
            if shape == "default":
                hl.profile_enable(True)
                hl.batch_run(pos[id(hl)], a.steps, stages=7 | binding.REPLAY_BAG, sync=True)
                rep = hl.profile_report()
                hl.profile_enable(False)
                row["loc_kernels"] = {k: [round(v[0], 3), v[1]] for k, v in sorted(rep.items(), key=lambda kv: -kv[1][0])}
            hl.close()
            hs.close()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
