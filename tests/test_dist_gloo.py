"""-m "not gpu": the N>1 path of bench.py (stream sharding, barrier, max-over-ranks) with world_size 2 on gloo."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from alego_loader import load_package
    load_package()
    from alego_amd import dist as D, synth
    from oracle import oracle_py as O
    dist = D.init("gloo")
    assert D.env() == (rank, rank, world)
    B = 2
    ids = D.stream_ids(rank, B)
    p = synth.default_params(16, 1800)
    poses = []
    for s in ids:  # the per-rank worker of this CPU test is the oracle; on GPUs it is the HIP handle
        o = O.Oracle(p)
        for k in range(3):
            o.process_scan(synth.scan(p, k, stream=s), stages=3)
        poses.append(o.get("odom_pose"))
    dist.barrier()
    dt = D.max_over_ranks(1.0 + rank, dist)  # rank 1 is "slower"
    gathered = [None] * world
    dist.all_gather_object(gathered, (ids, [x.tolist() for x in poses]))
    if rank == 0:
        q.put((dt, gathered, D.aggregate_scans_per_s(world, B, 3, dt)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_stream_sharding():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 400)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    dt, gathered, value = q.get(timeout=120)
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert dt == 2.0  # max over ranks
    ids = sum((g[0] for g in gathered), [])
    assert sorted(ids) == [0, 1, 2, 3]  # disjoint shards covering all streams
    poses = np.array(sum((g[1] for g in gathered), []))
    assert len({tuple(np.round(x, 9)) for x in poses}) == 4  # four different streams were really processed
    assert value == 2 * 2 * 3 / 2.0


def _shard_worker(rank, world, port, q):
    """One registration (BASELINE config 5): both ranks hold the same scans and map (replicated state); each evaluates its
    contiguous half of the residual rows, the 28 normal-equation scalars are all-reduced (gloo here, RCCL on the GPUs) and
    every rank takes the same trust-region steps."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from alego_loader import load_package
    load_package()
    from alego_amd import dist as D, synth
    from oracle import oracle_py as O
    import lm_control
    dist = D.init("gloo")
    p = synth.default_params(16, 1800)
    o = O.Oracle(p)
    x0 = None
    for k in range(16):          # every rank processes the same stream: identical (replicated) state
        if k == 15:
            x0 = o.get("lm_params").copy()
        o.process_scan(synth.scan(p, k))
    assert o.get("lm_info")[1] == 1, "scan 15 is a mapping frame with an optimisation"
    blocks = o.get("lm_blocks14").reshape(-1, 14)
    T = blocks.shape[0]
    mine = blocks[rank * T // world:(rank + 1) * T // world]      # this rank's slice of the rows
    n_allreduce = [0]

    def evaluate(x):
        part = torch.from_numpy(O.normal_eq(mine, x, p.huber_delta))
        dist.all_reduce(part)                                       # 28 doubles = 224 B per evaluation
        n_allreduce[0] += 1
        return part.numpy()

    x, info = lm_control.solve(evaluate, x0, p.lm_max_iters)
    x1, info1 = lm_control.solve(lambda xx: O.normal_eq(blocks, xx, p.huber_delta), x0, p.lm_max_iters)   # one rank, all rows
    xq, infoq = O.solve(np.concatenate([blocks[:, :1], blocks[:, 1:]], axis=1), x0, p.lm_max_iters, p.huber_delta)   # the oracle's DENSE_QR Ceres restatement
    gathered = [None] * world
    dist.all_gather_object(gathered, x.tolist())
    if rank == 0:
        q.put(dict(T=int(T), n_mine=int(mine.shape[0]), x=x.tolist(), x1=x1.tolist(), xq=xq.tolist(), info=info, info1=info1, infoq=infoq,
                   others=gathered, n_allreduce=n_allreduce[0]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_registration():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29100 + (os.getpid() % 400)
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    r = q.get(timeout=90)
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    x, x1, xq = np.array(r["x"]), np.array(r["x1"]), np.array(r["xq"])
    assert r["T"] > 500 and abs(r["n_mine"] - r["T"] / 2) <= 1
    assert np.array_equal(np.array(r["others"][0]), np.array(r["others"][1])), "both ranks must end with the identical pose"
    assert np.abs(x - x1).max() < 1e-9, "2-rank sum order vs 1-rank sum order"
    assert np.abs(x - xq).max() < 1e-4 and np.abs(x[3:] - xq[3:]).max() < 1e-4, (x, xq)      # north_star tolerance vs the QR-based oracle solve
    assert np.abs(x - xq).max() < 1e-6, "normal equations + Cholesky agree with DENSE_QR far inside the tolerance"
    assert r["info"]["iterations"] == r["infoq"]["iterations"] and r["info"]["termination"] == r["infoq"]["termination"]
    assert r["n_allreduce"] == 1 + r["info"]["iterations"] - 0 or r["n_allreduce"] <= 1 + r["info"]["iterations"]


def _shard_budget_worker(rank, world, port, q, outer, max_iter):
    """The registration of _shard_worker with LaserMapping's budgets at their edges: `outer` ceres::Solve calls in a row (each from the
    params_ the last one left, laserMapping.cpp:360), each with max_num_iterations = max_iter.  With a budget of 0 every solve is one
    evaluation at its start and returns it unchanged: the step that closes the outer iteration is its first one."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from alego_loader import load_package
    load_package()
    from alego_amd import dist as D, synth
    from oracle import oracle_py as O
    import lm_control
    dist = D.init("gloo")
    p = synth.default_params(16, 1800)
    o = O.Oracle(p)
    x0 = None
    for k in range(16):
        if k == 15:
            x0 = o.get("lm_params").copy()
        o.process_scan(synth.scan(p, k))
    blocks = o.get("lm_blocks14").reshape(-1, 14)
    T = blocks.shape[0]
    mine = blocks[rank * T // world:(rank + 1) * T // world]
    n_allreduce = [0]

    def evaluate(x):
        part = torch.from_numpy(O.normal_eq(mine, x, p.huber_delta))
        dist.all_reduce(part)
        n_allreduce[0] += 1
        return part.numpy()

    x, x1, xq = x0.copy(), x0.copy(), x0.copy()
    infos, infos1, infosq = [], [], []
    for _ in range(outer):
        x, info = lm_control.solve(evaluate, x, max_iter)
        x1, info1 = lm_control.solve(lambda xx: O.normal_eq(blocks, xx, p.huber_delta), x1, max_iter)
        xq, infoq = O.solve(blocks, xq, max_iter, p.huber_delta)
        infos.append(info); infos1.append(info1); infosq.append(infoq)
    gathered = [None] * world
    dist.all_gather_object(gathered, x.tolist())
    if rank == 0:
        q.put(dict(x0=x0.tolist(), x=x.tolist(), x1=x1.tolist(), xq=xq.tolist(), infos=infos, infos1=infos1, infosq=infosq,
                   others=gathered, n_allreduce=n_allreduce[0]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("outer,max_iter", [(3, 0), (2, 1)])
def test_two_rank_sharded_registration_budget_edges(outer, max_iter):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 28700 + (os.getpid() % 400) + 400 * max_iter
    procs = [ctx.Process(target=_shard_budget_worker, args=(r, 2, port, q, outer, max_iter)) for r in range(2)]
    [p.start() for p in procs]
    r = q.get(timeout=90)
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    x0, x, x1, xq = (np.array(r[k]) for k in ("x0", "x", "x1", "xq"))
    assert np.array_equal(np.array(r["others"][0]), np.array(r["others"][1])), "both ranks must end with the identical pose"
    assert np.abs(x - x1).max() < 1e-9, "2-rank sum order vs 1-rank sum order"
    assert np.abs(x - xq).max() < 1e-6, (x, xq)
    for i, (a, b) in enumerate(zip(r["infos"], r["infosq"])):
        assert (a["iterations"], a["successful"], a["termination"]) == (b["iterations"], b["successful"], b["termination"]), (i, a, b)
        assert a["iterations"] <= max_iter
    n_eval = sum(1 + a["iterations"] for a in r["infos"])
    assert r["n_allreduce"] == n_eval <= outer * (1 + max_iter), "one all-reduce per evaluation, within the worst-case sequence the host enqueues"
    if max_iter == 0:
        assert np.array_equal(x, x0) and np.array_equal(xq, x0), "a budget of 0 evaluates and leaves params_ as they were"
        assert all(a["termination"] == 0 and a["initial_cost"] == r["infos"][0]["initial_cost"] for a in r["infos"])
    else:
        assert not np.array_equal(x, x0), "the solves moved params_"
