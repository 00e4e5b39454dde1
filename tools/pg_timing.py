"""Wall time of the device pose-graph optimisation with correctPoses (alego_graph_optimize with apply = 1) against
(a) the numpy / scipy restatement of the same objective on one host core (tests/pose_graph_ref.py) and (b) the per-slot write-back
sequence a host pose graph has to use otherwise (alego_map_set_keyposes, alego_lm_set_keypose per resident frame,
alego_lm_reset_window, alego_lm_apply_correction).

A handle of max(--slots) slots replays the 560-scan synthetic lap from varied start scans for --steps scans with the archive and the
graph on; alego_loop_search finds the loops and every accepted one is added ONCE, so every timed graph has one loop edge.  For every N of
--slots the synchronous optimise call over the first N slots with a loop is timed with apply = 0 (median over --reps calls: the same
problem every time).  Then optimise + apply is timed once per size on disjoint windows of slots that have not been applied yet (1, 64,
256 slots and the rest), since an apply clears loop_closed_ and moves the poses.  Host wall time is device-synchronised time.  The same for
one constructed drifted circle of --big poses.

    python tools/pg_timing.py [--slots 1,64,256,1024] [--steps 420] [--reps 3] [--single 8] [--big 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alego_loader import load_package  # noqa: E402

load_package()
from alego_amd import binding, synth  # noqa: E402
import pose_graph_ref as R  # noqa: E402

LAP = 560


def graph_of(h, slot):
    c, l = h.graph_get_edges(0, slot=slot), h.graph_get_edges(1, slot=slot)
    return R.Graph(np.concatenate([c["frm"], l["frm"]]), np.concatenate([c["to"], l["to"]]), np.concatenate([c["between"], l["between"]]),
                   np.concatenate([c["variance"], l["variance"]]))


def archived_poses(h, slot):
    return np.array([h.map_get_keyframe(j, slot=slot)["pose"] for j in range(h.map_status(slot)[0])], np.float32).reshape(-1, 6)


def by_hand(h, slot, est, corr, K):
    poses = R.to_pose6(est)
    n = len(poses)
    h.map_set_keyposes(0, poses, slot=slot)
    for kf in range(max(0, n - K), n):
        h.lm_set_keypose(kf, poses[kf], slot=slot)
    h.lm_reset_window(slot=slot)
    h.lm_apply_correction(np.asarray(corr, np.float64).reshape(4, 4)[:3, :], slot=slot)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64,256,1024")
    ap.add_argument("--steps", type=int, default=420)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--single", type=int, default=8)
    ap.add_argument("--big", type=int, default=2000)
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
    h.graph_enable(2)
    h.batch_run(0, a.steps, stages=7 | binding.REPLAY_BAG, sync=True)
    found = h.loop_search(list(range(n)))
    closed = [s for s in range(n) if found[s]["status"] == 2]
    h.graph_add_loops(closed, [found[s] for s in closed])
    rows = []
    for N in sizes:
        sl = closed[:N]
        t, res = [], None
        for _ in range(a.reps):
            dt, res = timed(lambda: h.graph_optimize(sl))
            t.append(dt)
        assert all(r["status"] == 2 and r["n_loops"] == 1 for r in res)
        rows.append(dict(slots=len(sl), optimize_ms=1e3 * float(np.median(t)), optimize_ms_per_slot=1e3 * float(np.median(t)) / len(sl),
                         iterations=max(r["iterations"] for r in res), poses=float(np.mean([r["n_poses"] for r in res]))))
    # (a) the restatement on one core, on the first --single slots with a loop, from the same poses the device started from
    host = []
    for s in closed[:a.single]:
        g = graph_of(h, s)
        X0 = R.from_pose6(archived_poses(h, s))
        dt, _ = timed(lambda: g.optimize(X0))
        host.append(dt)
    first = 0
    for i, N in enumerate(sizes):
        sl = closed[first:first + N] if i + 1 < len(sizes) else closed[first:]
        first += len(sl)
        if not sl:
            continue
        dt, res = timed(lambda: h.graph_optimize(sl, apply=True))
        assert all(r["status"] == 2 and r["applied"] == 1 for r in res), [r for r in res if r["applied"] != 1][:3]
        rows[i].update(apply_slots=len(sl), with_apply_ms=1e3 * dt, with_apply_ms_per_slot=1e3 * dt / len(sl))
    # (b) the per-slot write-back of the same estimates
    hand = []
    K = p.recent_keyframe_num
    for s in closed[:a.single]:
        est = h.graph_get_estimate(slot=s)
        dt, _ = timed(lambda: by_hand(h, s, est, found[s]["T"], K))
        hand.append(dt)
    h.close()
    host_ms, hand_ms = 1e3 * float(np.median(host)), 1e3 * float(np.median(hand))
    # one large constructed graph: a drifted circle with one loop edge
    import test_pose_graph as T
    X0, g, _ = T.drifted_circle(a.big, 0.028 * 2000 / a.big, loops=((-1, 2),), loop_var=0.1)
    hb = T._constructed_handle([(X0, g)], 2, a.big)
    T._add_loops(hb, 0, g, len(X0))
    tb = []
    for _ in range(a.reps):
        dt, res = timed(lambda: hb.graph_optimize([0]))
        tb.append(dt)
    big_res = res[0]
    big_apply_s, res = timed(lambda: hb.graph_optimize([0], apply=True))
    assert res[0]["applied"] == 1, res
    hb.close()
    dt_host, (_, steps, _) = timed(lambda: g.optimize(X0))
    print("| slots (one loop edge each) | poses per slot | optimise (ms) | per slot (ms) | iterations | optimise + apply (ms per slot, slots) | restatement, 1 core (ms per slot) | per-slot write-back (ms per slot) |")
    print("|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        wa = f"{r['with_apply_ms_per_slot']:.3f} ({r['apply_slots']})" if "apply_slots" in r else "-"
        print(f"| {r['slots']} | {r['poses']:.0f} | {r['optimize_ms']:.2f} | {r['optimize_ms_per_slot']:.3f} | {r['iterations']} | {wa} | {host_ms:.2f} | {hand_ms:.2f} |")
    print(f"| 1 constructed | {a.big} | {1e3 * float(np.median(tb)):.2f} | {1e3 * float(np.median(tb)):.3f} | {big_res['iterations']} | {1e3 * big_apply_s:.2f} (1) | {1e3 * dt_host:.2f} ({len(steps)} steps) | - |")
    print(json.dumps(dict(rows=rows, host_ms_per_slot=host_ms, hand_ms_per_slot=hand_ms, big=dict(poses=a.big, optimize_ms=1e3 * float(np.median(tb)), with_apply_ms=1e3 * big_apply_s,
                                                                                              result=big_res, host_ms=1e3 * dt_host, host_steps=len(steps)), steps=a.steps, reps=a.reps)))


if __name__ == "__main__":
    main()
