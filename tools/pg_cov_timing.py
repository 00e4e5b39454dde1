"""Wall time of the key-pose graph's marginal covariances and of the loop-edge gate (alego_graph_marginals, alego_graph_check_edges; DESIGN.md
section 20) against (a) numpy's dense inverse of Lambda = J^T J on one host core and (b) one Gauss-Newton step of alego_graph_optimize of the
same build on the same graphs.

A handle of max(--slots) slots replays the 560-scan synthetic lap from varied start scans for --steps scans with the archive and the graph on;
alego_loop_search finds the loops and every accepted one is added once (38 poses and one loop edge per slot).  For every N of --slots the
synchronous calls over the first N such slots are timed: marginals, a check of 1 and of 8 candidates per slot, one optimise step.  The calls
are alternated --reps times and the medians reported; host wall time is device-synchronised time.  The same for one constructed drifted
circle of --big poses with one loop edge, whose marginals are also compared with the dense inverse (the difference is printed as a fraction of
eps * cond, which is above the 1e-4 the tests allow themselves at 1000 poses and beyond).

    python tools/pg_cov_timing.py [--slots 1,64,1024] [--steps 420] [--reps 5] [--single 8] [--big 2000] [--no-dense-big]
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
VAR = np.full(6, 0.01)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def alternated(calls, reps):
    """{name: median ms} of the calls run one after the other, reps times"""
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t[k].append(timed(fn)[0])
    return {k: 1e3 * float(np.median(v)) for k, v in t.items()}


def one_core():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def dense_inverse(g, X):
    _, J = g.jacobian(X)
    lam = (J.T @ J).toarray()
    with one_core():
        dt, sigma = timed(lambda: np.linalg.inv(lam))
    return dt, lam, sigma


def graph_of(h, slot):
    c, l = h.graph_get_edges(0, slot=slot), h.graph_get_edges(1, slot=slot)
    return R.Graph(np.concatenate([c["frm"], l["frm"]]), np.concatenate([c["to"], l["to"]]), np.concatenate([c["between"], l["between"]]),
                   np.concatenate([c["variance"], l["variance"]]))


def archived_poses(h, slot):
    return np.array([h.map_get_keyframe(j, slot=slot)["pose"] for j in range(h.map_status(slot)[0])], np.float32).reshape(-1, 6)


def candidates(slots, n_poses, frm, to, between, per):
    """per candidates for every slot: the pair (frm - k, to + k), all with the same measurement (any measurement costs the same)"""
    s, f, t, b = [], [], [], []
    for i, slot in enumerate(slots):
        for k in range(per):
            a, c = max(frm[i] - k, 0), min(to[i] + k, n_poses[i] - 1)
            if a == c:
                a, c = n_poses[i] - 1, 0
            s.append(slot); f.append(a); t.append(c); b.append(between[i])
    return s, f, t, b, [VAR] * len(s)


def check_call(h, s, f, t, b, v):
    """the candidates marshalled once: the timed call is alego_graph_check_edges alone"""
    sl = np.ascontiguousarray(s, np.int32)
    e, out = binding.graph_edges(f, t, b, v), (binding.GraphCheck * len(sl))()

    def call():
        rc = binding.lib().alego_graph_check_edges(h._h, sl.ctypes.data, len(sl), e, out)
        assert rc == 0 and out[0].status == 1, (rc, out[0].status)
    return call


def marginals_call(h, slots, cap):
    sl = np.ascontiguousarray(slots, np.int32)
    cov, out = np.zeros((len(sl), cap, 36)), (binding.GraphCovResult * len(sl))()

    def call():
        rc = binding.lib().alego_graph_marginals(h._h, sl.ctypes.data, len(sl), cap, cov.ctypes.data, out)
        assert rc == 0 and out[0].status == 1, (rc, out[0].status)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64,1024")
    ap.add_argument("--steps", type=int, default=420)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", type=int, default=8)
    ap.add_argument("--big", type=int, default=2000)
    ap.add_argument("--no-dense-big", action="store_true")
    a = ap.parse_args()
    sizes = [int(v) for v in a.slots.split(",") if int(v) > 0]
    p = synth.default_params(16, 1800)
    n = max(sizes + [0])
    rows = []
    if n > 0:
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
        for N in sizes:
            sl = closed[:N]
            npo = [h.map_status(s)[0] for s in sl]
            c1 = candidates(sl, npo, [found[s]["latest_id"] for s in sl], [found[s]["closest_id"] for s in sl], [found[s]["between"] for s in sl], 1)
            c8 = candidates(sl, npo, [found[s]["latest_id"] for s in sl], [found[s]["closest_id"] for s in sl], [found[s]["between"] for s in sl], 8)
            cap = max(npo)
            ms = alternated(dict(marginals=marginals_call(h, sl, cap), check1=check_call(h, *c1), check8=check_call(h, *c8),
                                 optimize_step=lambda: h.graph_optimize(sl, max_iters=1)), a.reps)
            rows.append(dict(slots=len(sl), poses=float(np.mean(npo)), **ms))
        dense = []
        for s in closed[:a.single]:
            dense.append(dense_inverse(graph_of(h, s), R.from_pose6(archived_poses(h, s)))[0])
        h.close()
        dense_ms = 1e3 * float(np.median(dense))
    import test_pose_graph as T
    X0, g, _ = T.drifted_circle(a.big, 0.028 * 2000 / a.big, loops=((-1, 2),), loop_var=0.1)
    hb = T._constructed_handle([(X0, g)], 2, a.big)
    T._add_loops(hb, 0, g, len(X0))
    N = len(X0)
    between = R.between(X0[N - 1], X0[3])
    c1 = candidates([0], [N], [N - 1], [3], [between], 1)
    c8 = candidates([0], [N], [N - 1], [3], [between], 8)
    big = alternated(dict(marginals=marginals_call(hb, [0], N), check1=check_call(hb, *c1), check8=check_call(hb, *c8),
                          optimize_step=lambda: hb.graph_optimize([0], max_iters=1)), a.reps)
    _, cov = hb.graph_marginals([0], cap=N)
    X = R.from_pose6(archived_poses(hb, 0))
    hb.close()
    big.update(poses=N)
    if not a.no_dense_big:
        dt, lam, sigma = dense_inverse(g, X)
        w = np.linalg.eigvalsh(lam)   # symmetric positive definite: cond = largest / smallest eigenvalue
        cond = float(w[-1] / w[0])
        frac = max(np.abs(cov[0, k] - sigma[6 * k:6 * k + 6, 6 * k:6 * k + 6]).max() / (2.2e-16 * cond * np.abs(sigma[6 * k:6 * k + 6, 6 * k:6 * k + 6]).max()) for k in range(N))
        big.update(dense_ms=1e3 * dt, cond=cond, fraction_of_eps_cond=float(frac))
    print("| slots | poses per slot | marginals (ms) | check, 1 candidate per slot (ms) | check, 8 per slot (ms) | one optimise step (ms) | dense inverse, 1 core (ms per slot) |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['slots']} | {r['poses']:.0f} | {r['marginals']:.2f} | {r['check1']:.2f} | {r['check8']:.2f} | {r['optimize_step']:.2f} | {dense_ms:.2f} |")
    print(f"| 1 constructed | {N} | {big['marginals']:.2f} | {big['check1']:.2f} | {big['check8']:.2f} | {big['optimize_step']:.2f} | {big.get('dense_ms', float('nan')):.0f} |")
    print(json.dumps(dict(rows=rows, dense_ms_per_slot=dense_ms if rows else None, big=big, steps=a.steps, reps=a.reps)))


if __name__ == "__main__":
    main()
