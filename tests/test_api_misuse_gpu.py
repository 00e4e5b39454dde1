"""-m gpu: what the host API answers to misuse, call by call, and whose profiler a launch is timed into.

The refusal table: every batched call and every *_enable, one case per single fault (the feature off, the wrong kind of handle, a slot -1 and a slot
n_slots, a slot or pair listed twice where that is refused, a self pair, a non-finite transform or option, n = 0), on handles of 2 or 3 slots at geometry
16 x 1800.  The cases are those of tools/api_refusals.py; the return code and the exact text of alego_last_error are written out below.  They were
recorded by that tool on the commit before the gate (csrc/api_gate.h) existed — profiles/r17_api_gate.md keeps that table — except that
alego_graph_optimize, alego_graph_marginals and alego_regcov_get now name the slot that is listed twice, as the other calls always did.  After every
refused call all slots of the mapping handle are byte-unchanged (test_map_merge.snap).

Profiler ownership: two handles driven from one thread; a launch is timed into the profiler of the handle the call was made on, whatever handle
the thread used before, and a handle outlives the other one's destruction."""
import importlib.util
import os

import numpy as np
import pytest

from alego_amd import binding
from test_map_merge import same, snap

_spec = importlib.util.spec_from_file_location("api_refusals", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "api_refusals.py"))
api_refusals = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(api_refusals)

ARG = binding.ERR_ARG
OFF_ARCHIVE = "the key-frame archive is off (alego_map_enable)"
OFF_ARCHIVE_FIRST = "the key-frame archive is off (alego_map_enable first)"
OFF_GRAPH = "the key-pose graph is off (alego_map_enable, then alego_graph_enable)"
OFF_APPEARANCE = "the appearance search is off (alego_map_enable, then alego_loop_appearance_enable)"
OFF_RELOC = "relocalisation is off (alego_loc_enable, then alego_reloc_enable)"
LOCALISING = "not available on a localising handle (alego_loc_enable)"
STREAM = "not available with alego_stream_setup"
RANGE = "slot out of range"
TWICE_1 = "slot 1 is listed twice"
N_CAND = "n_cand is 1 .. ALEGO_RELOC_MAX_CAND, verify 0 .. n_cand"
GRAPH_CHECK = "=graph check: measurement not finite or variance not positive and finite"
NO_TEXT = "=-"       # the call returns the code and sets no text of its own
MAP_NOT_MAPPING = "the key-frame archive / key-pose graph belong to a mapping handle"
USED = "call it before the first scan of any slot"
MAP_RANGE = "slot out of range of the mapping handle"

# call -> {fault: text}; the text follows "alego_<call>: " unless it starts with "=".  Every fault returns ALEGO_ERR_ARG; "n = 0" is accepted (code 0).
EXPECTED = {
    "loop_search": {"feature off": OFF_ARCHIVE, "wrong kind of handle": OFF_ARCHIVE, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None},
    "loop_search_appearance": {"feature off": OFF_APPEARANCE, "wrong kind of handle": OFF_APPEARANCE, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                               "a slot listed twice": TWICE_1, "n_cand too large": N_CAND, "verify > n_cand": N_CAND},
    "graph_add_loops": {"feature off": OFF_GRAPH, "wrong kind of handle": OFF_GRAPH, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None},
    "graph_optimize": {"feature off": OFF_GRAPH, "wrong kind of handle": OFF_GRAPH, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                       "a slot listed twice": TWICE_1},          # before the gate: "a slot is listed twice"
    "graph_marginals": {"feature off": OFF_GRAPH, "wrong kind of handle": OFF_GRAPH, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                        "a slot listed twice": TWICE_1,         # before the gate: "a slot is listed twice"
                        "cap = 0": NO_TEXT},
    "graph_check_edges": {"feature off": OFF_GRAPH, "wrong kind of handle": OFF_GRAPH, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                          "a measurement not finite": GRAPH_CHECK, "a variance not finite": GRAPH_CHECK},
    "graph_check_loops": {"feature off": OFF_GRAPH, "wrong kind of handle": OFF_GRAPH, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None},
    "regcov_get": {"feature off": "the feature is off (alego_regcov_enable)", "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                   "a slot listed twice": TWICE_1},              # before the gate: "a slot is listed twice"
    "loc_relocalize": {"feature off": OFF_RELOC, "wrong kind of handle": OFF_RELOC, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                       "a slot listed twice": TWICE_1, "n_cand too large": N_CAND, "verify > n_cand": N_CAND},
    "map_move": {"feature off": OFF_ARCHIVE, "wrong kind of handle": LOCALISING, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                 "a slot listed twice": TWICE_1, "a transform not finite": "a transform is not finite"},
    "map_thin": {"feature off": OFF_ARCHIVE, "wrong kind of handle": LOCALISING, "slot -1": RANGE, "slot n_slots": RANGE, "n = 0": None,
                 "a slot listed twice": TWICE_1, "min_dist NaN": "min_dist is not finite", "min_dist infinite": "min_dist is not finite"},
    "map_align": {"feature off": OFF_APPEARANCE, "wrong kind of handle": LOCALISING, "source -1": RANGE, "destination n_slots": RANGE,
                  "a self pair": "slot 2 is paired with itself", "a pair listed twice": "the pair (0, 1) is listed twice", "n = 0": None,
                  "n_queries too large": "n_queries is 1 .. ALEGO_ALIGN_MAX_QUERIES, n_cand 1 .. ALEGO_RELOC_MAX_CAND",
                  "n_cand too large": "n_queries is 1 .. ALEGO_ALIGN_MAX_QUERIES, n_cand 1 .. ALEGO_RELOC_MAX_CAND"},
    "map_merge": {"feature off": OFF_ARCHIVE, "wrong kind of handle": LOCALISING, "source -1": RANGE, "destination n_slots": RANGE,
                  "a self pair": "slot 2 is paired with itself", "a pair listed twice": "slot 1 is a destination twice", "n = 0": None,
                  "a destination listed twice": "slot 2 is a destination twice",
                  "a destination that is a source": "slot 1 is a destination of one pair and a source of another",
                  "a transform not finite": "a transform is not finite", "stamp_offset infinite": "stamp_offset is not finite",
                  "seam_variance NaN": "seam_variance must be positive and finite", "seam_variance zero": "seam_variance must be positive and finite"},
    "map_enable": {"after alego_stream_setup": STREAM, "wrong kind of handle": LOCALISING, "a second call": "already enabled", "max_keyframes 0": NO_TEXT},
    "graph_enable": {"feature off": OFF_ARCHIVE_FIRST, "wrong kind of handle": OFF_ARCHIVE_FIRST, "a second call": "already enabled"},
    "loop_appearance_enable": {"feature off": OFF_ARCHIVE_FIRST, "wrong kind of handle": LOCALISING, "a second call": "already enabled"},
    "regcov_enable": {"a second call": "already enabled", "an option not finite": "an option is not finite, or var_min exceeds var_max",
                      "graph = 1 with the graph off": "graph = 1 needs the key-pose graph (alego_graph_enable first)"},
    "loc_enable": {"after alego_stream_setup": STREAM, "wrong kind of handle": MAP_NOT_MAPPING, "after the first scan": USED, "a second call": "already enabled"},
    "loc_enable_from_map": {"after alego_stream_setup": STREAM, "wrong kind of handle": MAP_NOT_MAPPING, "after the first scan": USED,
                            "the mapping handle null": "the mapping handle is null",
                            "the mapping handle is the handle": "the mapping handle and the localising handle are the same",
                            "a mapping handle without archive": "the mapping handle has no key-frame archive (alego_map_enable)",
                            "slot -1 of the mapping handle": MAP_RANGE, "slot n_slots of the mapping handle": MAP_RANGE},
    "loc_update_from_map": {"wrong kind of handle": "the handle does not localise (alego_loc_enable / alego_loc_enable_from_map)",
                            "slot n_slots of the mapping handle": MAP_RANGE},
    "reloc_enable": {"feature off": "the handle does not localise (alego_loc_enable)", "wrong kind of handle": "the handle does not localise (alego_loc_enable)",
                     "a second call": "already enabled"},
    "trajectory_enable": {"after alego_stream_setup": STREAM + " (the poses of a look-ahead stream live in its lanes)", "capacity 0": NO_TEXT},
    "stream_setup": {"wrong kind of handle": LOCALISING},
}


def expected(name):
    call, fault = name.split(": ", 1)
    text = EXPECTED[call][fault]
    if text is None:
        return 0, ""
    return ARG, (text[1:] if text.startswith("=") else f"alego_{call}: {text}")


@pytest.mark.gpu
def test_every_refusal_has_its_code_and_text_and_changes_nothing():
    cases = api_refusals.cases()
    assert sorted(n for n, _, _ in cases) == sorted(f"{c}: {f}" for c, faults in EXPECTED.items() for f in faults), "the tool's cases and the table differ"
    S = api_refusals.build_scenes()
    try:
        m = S["mapper"]
        before = {s: snap(m, s) for s in range(api_refusals.N_MAP)}
        assert [m.map_status(s)[0] for s in range(api_refusals.N_MAP)] == [api_refusals.FRAMES, api_refusals.FRAMES, 0]
        wrong = []
        for name, scene, call in cases:
            got = api_refusals.answer(S, scene, call)
            print(f"{name} | {got[0]} | {got[1]}")
            if got != expected(name):
                wrong.append((name, got, expected(name)))
            for s in range(api_refusals.N_MAP):
                same(before[s], snap(m, s), f"after '{name}': slot {s} of the mapping handle")
        assert not wrong, wrong
    finally:
        api_refusals.close_scenes(S)


@pytest.mark.gpu
def test_a_launch_is_timed_into_its_own_handles_profiler():
    """On the commit before the gate the first two assertions fail: alego_debug_atan2f left the thread's profiler pointer where the previous call
    (on the other handle) had put it."""
    from alego_amd import synth
    p = synth.default_params(16, 1800)
    rng = np.random.default_rng(5)
    pts = np.c_[rng.uniform(-2, 2, (50, 3)), np.zeros(50)].astype(np.float32)
    y, x = rng.uniform(-3, 3, 64).astype(np.float32), rng.uniform(-3, 3, 64).astype(np.float32)
    A, B = binding.Handle(p), binding.Handle(p)
    try:
        A.profile_enable(True)
        assert len(A.voxel_grid(pts, 0.5)) > 0
        first = B.atan2f(y, x)
        rep = A.profile_report()
        assert rep and "atan2f_probe" not in rep, rep
        A.profile_enable(False)
        B.profile_enable(True)
        A.voxel_grid(pts, 0.5)
        B.atan2f(y, x)
        rep = B.profile_report()
        assert rep.get("atan2f_probe", (0.0, 0))[1] == 1 and set(rep) == {"atan2f_probe"}, rep
        A.close()
        last = B.atan2f(y, x)                  # an ordinary call on the surviving handle
        assert np.array_equal(first, last)
        assert np.abs(last.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 1e-6   # f32: an ulp at pi is 2.4e-7
    finally:
        A.close()
        B.close()
