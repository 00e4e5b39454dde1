"""Wall time of alego_map_thin next to the host sequence that rebuilds the kept frames in a fresh slot, on the archives
tools/map_merge_timing.py builds.

For every N of --slots a SLAM handle replays the 560-scan synthetic lap for --steps scans from varied start scans with the archive and the
key-pose graph on (22 - 23 frames per slot), with recent_keyframe_num = --recent: the newest recent + 1 frames are resident and always stay,
so the library's default of 50 would leave nothing to drop in archives this short.  A thin cannot be repeated on the same slot (nothing is
left to drop), so repetition r thins the fresh slots r N .. r N + N - 1 in one call.  In alternation, the host sequence is timed on the first
H = min(N, --host-slots) of them BEFORE the device call: alego_map_thin_select over the archived poses, alego_map_get_keyframe of every kept
frame, then alego_lm_reset_window, alego_lm_add_keyframe, alego_map_set_stamps, alego_map_thin_edges + alego_graph_set_edges in a fresh slot
(of a second handle: every slot of the first has replayed).  Host clock around the synchronous calls, medians over --reps; kernel times of
the last device call from alego_profile_report.  One JSON line per N.

    python tools/map_thin_timing.py [--slots 1,64] [--reps 5] [--steps 251] [--host-slots 64] [--min-dist 1.5] [--recent 4]
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


def host_thin(h, src, h2, dst, min_dist, K):
    n = h.map_status(src)[0]
    poses = np.array([h.map_get_keyframe(f, slot=src)["pose"] for f in range(n)], np.float32).reshape(-1, 6)
    protect = np.zeros(n, np.uint8)
    protect[:1] = 1
    protect[max(0, n - (K + 1)):] = 1
    lp = h.graph_get_edges(kind=1, slot=src)
    protect[np.r_[lp["frm"], lp["to"]].astype(int)] = 1
    keep = binding.map_thin_select(poses, protect, min_dist)
    ids = np.nonzero(keep)[0]
    frames = [h.map_get_keyframe(int(f), slot=src) for f in ids]
    stamps = h.map_get_stamps(slot=src)[ids]
    h2.lm_reset_window(slot=dst)
    for f in frames:
        h2.lm_add_keyframe(f["pose"], f["corner"], f["surf"], f["outlier"], slot=dst)
    h2.map_set_stamps(0, stamps, slot=dst)
    ch, lp = binding.map_thin_edges(h.graph_get_edges(kind=0, slot=src), lp, keep)
    h2.graph_set_edges(0, ch["frm"], ch["to"], ch["between"], ch["variance"], slot=dst)
    for i in range(len(lp["frm"])):
        h2.graph_add_edge(int(lp["frm"][i]), int(lp["to"][i]), lp["between"][i], lp["variance"][i], slot=dst)
    return len(ids)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=251)
    ap.add_argument("--host-slots", type=int, default=64)
    ap.add_argument("--min-dist", type=float, default=1.5)
    ap.add_argument("--recent", type=int, default=4)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    p.recent_keyframe_num = a.recent
    scans = [synth.scan(p, k) for k in range(LAP)]
    med = lambda v: round(float(np.median(v)), 4)
    for n in [int(v) for v in a.slots.split(",")]:
        nh = min(n, a.host_slots)
        n_slots = a.reps * n
        h = binding.Handle(p, n_slots=n_slots)
        h2 = binding.Handle(p, n_slots=a.reps * nh)
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, scans[k])
        for s in range(n_slots):
            h.replay_assign(s, 0, ((s % n) * 37) % LAP)    # every repetition thins the same N archives
        for x in (h, h2):
            x.map_enable(64, 1 << 19)
            x.graph_enable(4)
        h.batch_run(0, a.steps, stages=7 | binding.REPLAY_BAG, sync=False)
        h.synchronize()
        dev_ms, host_ms, res, kept = [], [], [], []
        for r in range(a.reps):
            slots = list(range(r * n, (r + 1) * n))
            host_ms.append(clock(lambda: kept.append([host_thin(h, slots[i], h2, r * nh + i, a.min_dist, a.recent) for i in range(nh)])))
            if r == a.reps - 1:   # the kernels of the last device call
                h.profile_enable(True)
            dev_ms.append(clock(lambda: res.append(h.map_thin(slots, a.min_dist))))
            if r == a.reps - 1:
                kernels = h.profile_report()
                h.profile_enable(False)
        last = res[-1]
        assert [x["frames"] for x in last[:nh]] == kept[-1], "the device keeps what the host sequence keeps"
        row = dict(slots=n, host_slots=nh, steps=a.steps, reps=a.reps, min_dist=a.min_dist, recent_keyframe_num=a.recent,
                   frames_before=[x["frames_before"] for x in last[:8]], frames=[x["frames"] for x in last[:8]],
                   points_before=int(np.mean([x["points_before"] for x in last])), points=int(np.mean([x["points"] for x in last])),
                   thinned=sum(x["status"] == 2 for x in last),
                   thin_ms=[round(v, 3) for v in dev_ms], thin_median_ms=med(dev_ms), thin_ms_per_slot=round(med(dev_ms) / n, 5),
                   host_ms=[round(v, 3) for v in host_ms], host_ms_per_slot=round(med(host_ms) / nh, 4))
        row["thin_kernels_ms"] = {k: round(v[0], 4) for k, v in kernels.items() if k.startswith(("th_", "mg_", "pg_", "vox", "lm_"))}
        h.close()
        h2.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
