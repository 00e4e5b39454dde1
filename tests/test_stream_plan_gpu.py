"""-m gpu: a handle whose streams were fitted to few hardware queues (csrc/stream_plan.h) computes what one with queues to spare computes.

ALEGO_HW_QUEUES is the budget the plan is fitted to; it is set only around handle creation, and the queue count of the process itself is left
alone.  The plan decides which HIP stream a kernel is enqueued on and nothing else, so every comparison is bit for bit."""
import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

CHECK_ARRAYS = ("seg_cloud", "seg_col", "less_sharp", "less_flat", "lm_corner_map_ds", "lm_surf_map_ds")   # what bench.py's timed_handle_check compares
NSLOT, NSCAN = 5, 30   # 30 scans: key frames, a rebuilt local map, and both waits of the hand-over (the scan two back, the scan before)


def _state(h, slot):
    _, odom, mp = h.batch_get_pose(slot)
    out = {f"odom {k}": odom[k] for k in ("t", "q")}
    out.update({f"map {k}": mp[k] for k in ("t", "q", "params")})
    out.update({name: h.debug_get(name, slot=slot) for name in CHECK_ARRAYS})
    return out


def _batch(p, n_slots, streams):
    h = binding.Handle(p, n_slots=n_slots, ring_len=NSCAN)
    for s, stream in enumerate(streams):
        for k in range(NSCAN):
            h.batch_load(s, k, synth.scan(p, k, stream=stream))
    return h


@pytest.fixture(scope="module")
def one_slot_states(params_a):
    """every stream alone on a one-slot handle, computed once"""
    ref = []
    for s in range(NSLOT):
        h = _batch(params_a, 1, [s])
        h.batch_run(0, NSCAN, stages=7)
        ref.append(_state(h, 0))
        assert h.batch_get_counts(0)["n_rebuild"] >= 1, "the scans were meant to rebuild the local map"
        h.close()
    return ref


@pytest.mark.parametrize("queues,lm_async", [(3, False), (6, True)])
def test_batch_results_do_not_depend_on_the_queue_budget(params_a, one_slot_states, queues, lm_async, monkeypatch):
    """5 slots in groups of 2 + 2 + 1: with 3 queues LaserMapping follows the front end on the group's one stream, with 6 it runs on the
    group's back stream.  Both give every slot the poses, LM params_ and clouds of the one-slot handles (hence of each other)."""
    monkeypatch.setenv("ALEGO_STREAM_GROUPS", "3")
    monkeypatch.setenv("ALEGO_HW_QUEUES", str(queues))
    monkeypatch.delenv("ALEGO_LM_ASYNC", raising=False)
    h = _batch(params_a, NSLOT, range(NSLOT))
    monkeypatch.delenv("ALEGO_STREAM_GROUPS")
    monkeypatch.delenv("ALEGO_HW_QUEUES")
    assert h.stream_plan() == dict(groups=3, slots_per_group=2, lm_async=lm_async, hw_queues=queues)
    assert h.stream_groups() == (3, 2)
    h.batch_run(0, NSCAN, stages=7)
    for s in range(NSLOT):
        got = _state(h, s)
        for name, want in one_slot_states[s].items():
            assert_bit_equal(got[name], want, f"{queues} queues, slot {s}: {name}")
    h.close()


@pytest.mark.parametrize("queues", [2, 4])
def test_stream_run_within_the_queue_budget_is_bit_identical(params_a, queues, monkeypatch):
    """alego_stream_run with two look-ahead lanes on min(3, Q) HIP streams (Q = 2: LaserOdometry and LaserMapping share the handle's back
    stream) against the serial one-slot replay of the same bag, pose by pose."""
    p = params_a
    bag_len = 12
    scans = [synth.scan(p, k) for k in range(bag_len)]
    ha = binding.Handle(p, n_slots=1, ring_len=1)
    monkeypatch.setenv("ALEGO_HW_QUEUES", str(queues))
    monkeypatch.delenv("ALEGO_STREAM_GROUPS", raising=False)
    monkeypatch.delenv("ALEGO_LM_ASYNC", raising=False)
    hb = binding.Handle(p, n_slots=5, ring_len=1)
    monkeypatch.delenv("ALEGO_HW_QUEUES")
    assert hb.stream_plan() == dict(groups=1, slots_per_group=5, lm_async=True, hw_queues=queues)
    for h in (ha, hb):
        h.replay_create(1, bag_len)
        for k, a in enumerate(scans):
            h.replay_load(0, k, a)
    ha.replay_assign(0, 0, 0)
    hb.stream_setup(0, 0)
    step = 0
    for n in (1, 2, 5, 4):   # 12 scans; 5: a call that ends inside a pair of lanes
        ha.batch_run(step, n, stages=7 | binding.REPLAY_BAG)
        hb.stream_run(step, n, stages=7)
        step += n
        fa, oa, ma = ha.batch_get_pose(0)
        fb, ob, mb = hb.batch_get_pose(0)
        for k in ("t", "q", "params"):
            assert_bit_equal(ob[k], oa[k], f"{queues} queues, after {step} scans: odometry {k}")
            assert_bit_equal(mb[k], ma[k], f"{queues} queues, after {step} scans: map {k}")
        assert fa == fb, (fa, fb)
    assert np.array_equal(hb.debug_get("lm_surf_map_ds"), ha.debug_get("lm_surf_map_ds"))
    ha.close(); hb.close()
