"""Wall time of alego_map_merge and alego_map_move next to the host sequences that define them, on one handle.

For every N of --pairs a SLAM handle replays the 560-scan synthetic lap for --steps scans from varied start scans with the archive and the
key-pose graph on (section 17's archives: 22 - 23 frames per slot).  Slots 0 .. N - 1 are the sources.  A merge cannot be repeated on the same
destination (its archive grows), so every repetition takes fresh destinations, which hold an archive of their own: with H = min(N, --host-pairs),
repetition r merges source i into slot N + r (N + H) + i on the device and, in alternation, into slot N + r (N + H) + N + i through the defining host sequence
(alego_map_get_keyframe, alego_map_align_poses, alego_lm_add_keyframe, alego_map_set_stamps, alego_graph_set_edges).  --host-pairs caps the pairs
the host sequence is timed on (it is reported per pair).  The move is repeatable: the sources are moved by G and by G^-1 in turn, on the device
and through alego_map_set_keyposes + alego_lm_set_keypose + alego_lm_reset_window + alego_lm_apply_correction + alego_graph_set_edges.
Host clock around the synchronous calls, medians over --reps; kernel times from alego_profile_report.  One JSON line per N.

    python tools/map_merge_timing.py [--pairs 1,64,1024] [--reps 5] [--steps 251] [--host-pairs 64]
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
SEAM = [1e-2, 1e-2, 1e-2, 0.25, 0.25, 0.25]


def rigid(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, t[0]], [s, c, 0, t[1]], [0, 0, 1, t[2]]], np.float64)


def inverse(T):
    R = T[:, :3].T
    return np.c_[R, -R @ T[:, 3]]


def host_merge(h, src, dst, T):
    ns, nd = h.map_status(src)[0], h.map_status(dst)[0]
    frames = [h.map_get_keyframe(f, slot=src) for f in range(ns)]
    poses = binding.map_align_poses(T, np.array([f["pose"] for f in frames], np.float32))
    stamps = h.map_get_stamps(slot=src)
    h.lm_reset_window(slot=dst)
    for f in range(ns):
        h.lm_add_keyframe(poses[f], frames[f]["corner"], frames[f]["surf"], frames[f]["outlier"], slot=dst)
    h.map_set_stamps(nd, stamps, slot=dst)
    ch = h.graph_get_edges(kind=0, slot=src)
    if ns > 1:
        h.graph_set_edges(nd + 1, ch["frm"][1:] + nd, ch["to"][1:] + nd, ch["between"][1:], ch["variance"][1:], slot=dst)
    seam = h.graph_get_edges(kind=0, first=nd, n=1, slot=dst)
    h.graph_set_edges(nd, seam["frm"], seam["to"], seam["between"], [SEAM], slot=dst)


def host_move(h, s, T, K):
    n = h.map_status(s)[0]
    poses = binding.map_align_poses(T, np.array([h.map_get_keyframe(f, slot=s)["pose"] for f in range(n)], np.float32))
    h.map_set_keyposes(0, poses, slot=s)
    for kf in range(max(0, n - K), n):
        h.lm_set_keypose(kf, poses[kf], slot=s)
    h.lm_reset_window(slot=s)
    h.lm_apply_correction(T.reshape(12), slot=s)
    e = h.graph_get_edges(kind=0, first=0, n=1, slot=s)
    B = np.vstack([e["between"][0], [0, 0, 0, 1]])
    h.graph_set_edges(0, [-1], [0], [(np.vstack([T, [0, 0, 0, 1]]) @ B)[:3]], e["variance"], slot=s)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=251)
    ap.add_argument("--host-pairs", type=int, default=64)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    K = p.recent_keyframe_num
    scans = [synth.scan(p, k) for k in range(LAP)]
    med = lambda v: round(float(np.median(v)), 4)
    G = rigid(0.7, [30.0, -20.0, 1.5])
    for n in [int(v) for v in a.pairs.split(",")]:
        nh = min(n, a.host_pairs)
        n_slots = n + a.reps * (n + nh)
        h = binding.Handle(p, n_slots=n_slots)
        h.replay_create(1, LAP)
        for k in range(LAP):
            h.replay_load(0, k, scans[k])
        for s in range(n_slots):
            h.replay_assign(s, 0, (s * 37) % LAP)
        h.map_enable(64, 1 << 19)
        h.graph_enable(4)
        h.batch_run(0, a.steps, stages=7 | binding.REPLAY_BAG, sync=False)
        h.synchronize()
        frames = [h.map_status(s)[0] for s in range(min(n, 8))]
        points = int(np.mean([h.map_status(s)[2] for s in range(min(n, 64))]))
        dev_ms, host_ms, res = [], [], []
        for r in range(a.reps):
            base = n + r * (n + nh)
            pairs = [(i, base + i) for i in range(n)]
            if r == a.reps - 1:   # the kernels of the last device merge
                h.profile_enable(True)
            dev_ms.append(clock(lambda: res.append(h.map_merge(pairs, G, seam_variance=SEAM))))
            if r == a.reps - 1:
                merge_kernels = h.profile_report()
                h.profile_enable(False)
            host_ms.append(clock(lambda: [host_merge(h, i, base + n + i, G) for i in range(nh)]))
        mv_dev, mv_host = [], []
        src = list(range(n))
        for r in range(a.reps):
            for T in (G, inverse(G)):
                mv_dev.append(clock(lambda: h.map_move(src, T)))
                mv_host.append(clock(lambda: [host_move(h, s, T, K) for s in range(nh)]))
        row = dict(pairs=n, host_pairs=nh, steps=a.steps, reps=a.reps, frames_per_slot=frames, points_per_source=points,
                   merge_ms=[round(v, 3) for v in dev_ms], merge_median_ms=med(dev_ms), merge_ms_per_pair=round(med(dev_ms) / n, 5),
                   host_merge_ms=[round(v, 3) for v in host_ms], host_merge_ms_per_pair=round(med(host_ms) / nh, 4),
                   move_ms=[round(v, 3) for v in mv_dev], move_median_ms=med(mv_dev), move_ms_per_slot=round(med(mv_dev) / n, 5),
                   host_move_ms=[round(v, 3) for v in mv_host], host_move_ms_per_slot=round(med(mv_host) / nh, 4))
        row["merged"] = sum(x["status"] == 2 for x in res[-1])
        row["merge_kernels_ms"] = {k: round(v[0], 4) for k, v in merge_kernels.items() if k.startswith(("mg_", "pg_", "vox", "lm_"))}
        h.profile_enable(True)
        h.map_move(src, G)
        rep = h.profile_report()
        h.profile_enable(False)
        row["move_kernels_ms"] = {k: round(v[0], 4) for k, v in rep.items() if k.startswith(("mg_", "pg_", "vox", "lm_"))}
        h.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
