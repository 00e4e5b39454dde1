"""-m "not gpu": csrc/stream_plan.h — how many HIP streams a handle drives at a given number of hardware queues — as a program of its own.

tests/stream_plan/stream_plan_table.cpp prints the plan of every case; the expectations are here: the plan fits the queues wherever the caller
left the choice to the library, it is the formula of the rounds before the fit from 8 queues on, and explicit requests are taken as they are."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = (1, 3, 63, 64, 255, 256, 4096)
TABLE_Q4_4096 = (4, 1024, 0)   # profiles/r07_stream_plan.md: groups, slots per group, back streams at Q = 4 with 4 096 slots


def parent_plan(n_slots, req_groups):
    """alego_create before the fit: (groups, slots per group); LaserMapping's back streams were on unless ALEGO_LM_ASYNC=0"""
    g = n_slots // 64 if req_groups < 0 else req_groups
    g = max(1, min(g, 8, n_slots))
    if req_groups < 0:
        g = min(g, 4)
    per = -(-n_slots // g)
    return -(-n_slots // per), per


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the header includes no HIP: a host compiler alone builds it
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "stream_plan", "stream_plan_table.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("stream_plan ok"), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    plans, queues, look = {}, {}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "plan":
            plans[tuple(int(v) for v in w[1:5])] = tuple(int(v) for v in w[6:10])
        elif w[0] == "queue":
            queues[(w[1], w[2])] = int(w[4])
        elif w[0] == "look":
            look[(int(w[1]), int(w[2]))] = int(w[4])
    return plans, queues, look


def test_default_plan_fits_the_queues(table):
    plans = table[0]
    for q in range(1, 33):
        for n in SLOTS:
            g, per, a, qq = plans[(q, n, -1, -1)]
            assert qq == q
            assert g >= 1 and g * (1 + a) <= q, (q, n, g, a)
            assert 1 <= per and (g - 1) * per < n <= g * per, (q, n, g, per)   # contiguous groups cover every slot, none is empty
            assert g <= max(n // 64, 1) and g <= 4, (q, n, g)                  # never more groups than the request of n_slots / 64 capped at 4


def test_plan_is_the_parents_where_queues_suffice(table):
    plans = table[0]
    for q in range(8, 33):
        for n in SLOTS:
            assert plans[(q, n, -1, -1)][:3] == parent_plan(n, -1) + (1,), (q, n)
            for rg in range(0, 5):   # up to 4 requested groups their back streams fit as well
                assert plans[(q, n, rg, -1)][:3] == parent_plan(n, rg) + (1,), (q, n, rg)
                assert plans[(q, n, rg, 0)][:3] == parent_plan(n, rg) + (0,), (q, n, rg)


def test_explicit_requests_are_honoured(table):
    plans = table[0]
    for q in range(1, 33):
        for n in SLOTS:
            for rg in range(0, 10):
                for ra in (0, 1):
                    assert plans[(q, n, rg, ra)][:3] == parent_plan(n, rg) + (ra,), (q, n, rg, ra)   # both given: the parent's plan at any Q
                g, per, a, _ = plans[(q, n, rg, -1)]
                assert (g, per) == parent_plan(n, rg) and a == int(2 * g <= q), (q, n, rg)           # groups given: back streams only where they fit
            for ra in (0, 1):
                g, per, a, _ = plans[(q, n, -1, ra)]
                assert a == ra and g >= 1 and (g - 1) * per < n <= g * per
                assert g * (1 + a) <= q or g == 1, (q, n, ra, g)                                      # back streams given: the groups make room
    assert plans[(4, 4096, 4, 1)][:3] == (4, 1024, 1) and plans[(2, 4096, 4, 1)][:3] == (4, 1024, 1)   # the A/B switch back to the parent's plan
    assert plans[(6, 5, 3, -1)][:3] == (3, 2, 1) and plans[(3, 5, 3, -1)][:3] == (3, 2, 0)              # 2 + 2 + 1 slots


def test_measured_table_entry(table):
    assert table[0][(4, 4096, -1, -1)][:3] == TABLE_Q4_4096


def test_queue_budget_sources(table):
    queues = table[1]
    assert queues[("-", "-")] == 4                                   # HIP's default
    assert queues[("-", "8")] == 8 and queues[("-", "2")] == 2       # GPU_MAX_HW_QUEUES, read only
    assert queues[("2", "8")] == 2 and queues[("32", "-")] == 32     # ALEGO_HW_QUEUES comes first
    for bad in ("0", "x", "-3"):
        assert queues[(bad, "8")] == 8 and queues[("-", bad)] == 4 and queues[(bad, bad)] == 4


def test_lookahead_stream_count(table):
    look = table[2]
    for q in range(1, 9):
        assert look[(q, 1)] == min(3, q)
        assert look[(q, 2)] == max(2, min(3, q))   # a back stream asked for explicitly stays in use
