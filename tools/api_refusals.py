"""What every batched call and every *_enable of the C ABI answers to a single fault: the return code and the text of alego_last_error.

The table is the behaviour a refactor of the host API has to keep: run it on the parent commit and on the head and diff the two outputs
(profiles/r17_api_gate.md holds both).  tests/test_api_misuse_gpu.py runs the same cases and asserts the table written out there.

Scenes (handles of 2 or 3 slots, geometry 16 x 1800):
    plain       nothing enabled
    mapper      archive, key-pose graph, appearance search and registration covariance on; three key frames in slots 0 and 1
    localiser   alego_loc_enable on an empty map, then alego_reloc_enable
    used        one scan processed
    stream      alego_stream_setup done
A call that sets no text of its own (a bare return of the code) is shown with the text "-": alego_last_error would repeat the previous failure's.

    python tools/api_refusals.py            # one line per case: name | code | text
    ALEGO_LIB=/path/to/another/libalego_mi355x.so python tools/api_refusals.py
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alego_loader import load_package  # noqa: E402

load_package()
from alego_amd import binding, synth  # noqa: E402

F32 = np.float32
N_MAP, N_LOC = 3, 2               # slots of the mapper / of the localiser
FRAMES = 3                        # key frames in slots 0 and 1 of the mapper
I34 = np.eye(3, 4)
VAR = np.full(6, 1e-4)
NAN, INF = float("nan"), float("inf")
SENTINEL = "unknown option api_refusals"


def _cloud(rng, n):
    return np.c_[rng.uniform(-20, 20, (n, 3)), rng.uniform(0, 16, (n, 1))].astype(F32)


def build_scenes():
    p = synth.default_params(16, 1800)
    rng = np.random.default_rng(17)
    S = {}
    S["plain"] = binding.Handle(p, n_slots=N_MAP)
    m = S["mapper"] = binding.Handle(p, n_slots=N_MAP)
    m.regcov_enable()
    m.map_enable(8, 4000)
    m.graph_enable(4)
    m.loop_appearance_enable()
    for s in (0, 1):
        for k in range(FRAMES):
            m.lm_add_keyframe(np.array([3.0 * k, s, 0, 0, 0, 0.1 * k], F32), _cloud(rng, 20), _cloud(rng, 60), _cloud(rng, 20), slot=s)
    loc = S["localiser"] = binding.Handle(p, n_slots=N_LOC)
    loc.loc_enable([], 0.0)
    loc.reloc_enable()
    u = S["used"] = binding.Handle(p, n_slots=1)
    u.scan_process(synth.scan(p, 0), stages=7)
    st = S["stream"] = binding.Handle(p, n_slots=3)
    st.replay_create(1, 2)
    for k in range(2):
        st.replay_load(0, k, synth.scan(p, k))
    st.stream_setup(0)
    return S


def close_scenes(S):
    for h in S.values():
        h.close()


def _loop():
    return dict(status=2, latest_id=2, closest_id=0, fitness=0.1, noise_variance=0.1, T=np.eye(4), between=I34)


def _list_cases(name, call, n, feature_off=(), wrong_kind=(), distinct=True):
    """the faults every call over a list of slots shares; call(handle, slots)"""
    out = [(f"{name}: {why}", scene, (lambda S, sc=scene: call(S[sc], [0]))) for why, scene in
           [("feature off", s) for s in feature_off] + [("wrong kind of handle", s) for s in wrong_kind]]
    ok = "localiser" if n == N_LOC else "mapper"
    out += [(f"{name}: slot -1", ok, lambda S: call(S[ok], [0, -1])),
            (f"{name}: slot n_slots", ok, lambda S: call(S[ok], [n])),
            (f"{name}: n = 0", ok, lambda S: call(S[ok], []))]
    if distinct:
        out.append((f"{name}: a slot listed twice", ok, lambda S: call(S[ok], [1, 0, 1])))
    return out


def cases():
    """(name, the scene whose handle the call is made on, call(scenes))"""
    T = np.broadcast_to(I34, (1, 3, 4)).copy()
    Tnan = T.copy(); Tnan[0, 1, 2] = NAN
    nanb = I34.copy(); nanb[1, 1] = NAN
    C = []
    C += _list_cases("loop_search", lambda h, s: h.loop_search(s), N_MAP, feature_off=["plain"], wrong_kind=["localiser"], distinct=False)
    C += _list_cases("loop_search_appearance", lambda h, s: h.loop_search_appearance(s), N_MAP, feature_off=["plain"], wrong_kind=["localiser"])
    C += [("loop_search_appearance: n_cand too large", "mapper", lambda S: S["mapper"].loop_search_appearance([0], n_cand=binding.RELOC_MAX_CAND + 1)),
          ("loop_search_appearance: verify > n_cand", "mapper", lambda S: S["mapper"].loop_search_appearance([0], n_cand=2, verify=3))]
    C += _list_cases("graph_add_loops", lambda h, s: h.graph_add_loops(s, [_loop() for _ in s]), N_MAP, feature_off=["plain"], wrong_kind=["localiser"], distinct=False)
    C += _list_cases("graph_optimize", lambda h, s: h.graph_optimize(s), N_MAP, feature_off=["plain"], wrong_kind=["localiser"])
    C += _list_cases("graph_marginals", lambda h, s: h.graph_marginals(s, cap=4), N_MAP, feature_off=["plain"], wrong_kind=["localiser"])
    C += [("graph_marginals: cap = 0", "mapper", lambda S: S["mapper"].graph_marginals([0], cap=0))]
    chk = lambda h, s: h.graph_check_edges(s, [2] * len(s), [0] * len(s), [I34] * len(s), [VAR] * len(s))
    C += _list_cases("graph_check_edges", chk, N_MAP, feature_off=["plain"], wrong_kind=["localiser"], distinct=False)
    C += [("graph_check_edges: a measurement not finite", "mapper", lambda S: S["mapper"].graph_check_edges([0], [2], [0], [nanb], [VAR])),
          ("graph_check_edges: a variance not finite", "mapper", lambda S: S["mapper"].graph_check_edges([0], [2], [0], [I34], [VAR * INF]))]
    C += _list_cases("graph_check_loops", lambda h, s: h.graph_check_loops(s, [_loop() for _ in s]), N_MAP, feature_off=["plain"], wrong_kind=["localiser"], distinct=False)
    C += _list_cases("regcov_get", lambda h, s: h.regcov_get(s), N_MAP, feature_off=["plain"])
    C += _list_cases("loc_relocalize", lambda h, s: h.loc_relocalize(s), N_LOC, feature_off=["plain"], wrong_kind=["mapper"])
    C += [("loc_relocalize: n_cand too large", "localiser", lambda S: S["localiser"].loc_relocalize([0], n_cand=binding.RELOC_MAX_CAND + 1)),
          ("loc_relocalize: verify > n_cand", "localiser", lambda S: S["localiser"].loc_relocalize([0], n_cand=2, verify=3))]
    C += _list_cases("map_move", lambda h, s: h.map_move(s, I34), N_MAP, feature_off=["plain"], wrong_kind=["localiser"])
    C += [("map_move: a transform not finite", "mapper", lambda S: S["mapper"].map_move([0], Tnan))]
    C += _list_cases("map_thin", lambda h, s: h.map_thin(s, 1.0), N_MAP, feature_off=["plain"], wrong_kind=["localiser"])
    C += [("map_thin: min_dist NaN", "mapper", lambda S: S["mapper"].map_thin([0], NAN)),
          ("map_thin: min_dist infinite", "mapper", lambda S: S["mapper"].map_thin([0], -INF))]
    for name, call in (("map_align", lambda h, pr: h.map_align(pr)), ("map_merge", lambda h, pr: h.map_merge(pr, I34))):
        C += [(f"{name}: feature off", "plain", lambda S, c=call: c(S["plain"], [(0, 1)])),
              (f"{name}: wrong kind of handle", "localiser", lambda S, c=call: c(S["localiser"], [(0, 1)])),
              (f"{name}: source -1", "mapper", lambda S, c=call: c(S["mapper"], [(-1, 1)])),
              (f"{name}: destination n_slots", "mapper", lambda S, c=call: c(S["mapper"], [(0, 1), (0, N_MAP)])),
              (f"{name}: a self pair", "mapper", lambda S, c=call: c(S["mapper"], [(0, 1), (2, 2)])),
              (f"{name}: a pair listed twice", "mapper", lambda S, c=call: c(S["mapper"], [(0, 1), (0, 2), (0, 1)])),
              (f"{name}: n = 0", "mapper", lambda S, c=call: c(S["mapper"], np.zeros((0, 2), np.int32)))]
    C += [("map_align: n_queries too large", "mapper", lambda S: S["mapper"].map_align([(0, 1)], n_queries=binding.ALIGN_MAX_QUERIES + 1)),
          ("map_align: n_cand too large", "mapper", lambda S: S["mapper"].map_align([(0, 1)], n_cand=binding.RELOC_MAX_CAND + 1)),
          ("map_merge: a destination listed twice", "mapper", lambda S: S["mapper"].map_merge([(0, 2), (1, 2)], I34)),
          ("map_merge: a destination that is a source", "mapper", lambda S: S["mapper"].map_merge([(0, 1), (1, 2)], I34)),
          ("map_merge: a transform not finite", "mapper", lambda S: S["mapper"].map_merge([(0, 2)], Tnan)),
          ("map_merge: stamp_offset infinite", "mapper", lambda S: S["mapper"].map_merge([(0, 2)], I34, stamp_offset=INF)),
          ("map_merge: seam_variance NaN", "mapper", lambda S: S["mapper"].map_merge([(0, 2)], I34, seam_variance=[1, 1, NAN, 1, 1, 1])),
          ("map_merge: seam_variance zero", "mapper", lambda S: S["mapper"].map_merge([(0, 2)], I34, seam_variance=[1, 1, 1, 0, 1, 1]))]
    # ---- the *_enable calls
    C += [("map_enable: after alego_stream_setup", "stream", lambda S: S["stream"].map_enable(8, 4000)),
          ("map_enable: wrong kind of handle", "localiser", lambda S: S["localiser"].map_enable(8, 4000)),
          ("map_enable: a second call", "mapper", lambda S: S["mapper"].map_enable(8, 4000)),
          ("map_enable: max_keyframes 0", "plain", lambda S: S["plain"].map_enable(0, 4000)),
          ("graph_enable: feature off", "plain", lambda S: S["plain"].graph_enable(4)),
          ("graph_enable: wrong kind of handle", "localiser", lambda S: S["localiser"].graph_enable(4)),
          ("graph_enable: a second call", "mapper", lambda S: S["mapper"].graph_enable(4)),
          ("loop_appearance_enable: feature off", "plain", lambda S: S["plain"].loop_appearance_enable()),
          ("loop_appearance_enable: wrong kind of handle", "localiser", lambda S: S["localiser"].loop_appearance_enable()),
          ("loop_appearance_enable: a second call", "mapper", lambda S: S["mapper"].loop_appearance_enable()),
          ("regcov_enable: a second call", "mapper", lambda S: S["mapper"].regcov_enable()),
          ("regcov_enable: an option not finite", "plain", lambda S: S["plain"].regcov_enable(binding.regcov_opts(sigma0=NAN))),
          ("regcov_enable: graph = 1 with the graph off", "plain", lambda S: S["plain"].regcov_enable(binding.regcov_opts(graph=1))),
          ("loc_enable: after alego_stream_setup", "stream", lambda S: S["stream"].loc_enable([], 0.0)),
          ("loc_enable: wrong kind of handle", "mapper", lambda S: S["mapper"].loc_enable([], 0.0)),
          ("loc_enable: after the first scan", "used", lambda S: S["used"].loc_enable([], 0.0)),
          ("loc_enable: a second call", "localiser", lambda S: S["localiser"].loc_enable([], 0.0)),
          ("loc_enable_from_map: after alego_stream_setup", "stream", lambda S: S["stream"].loc_enable_from_map(S["mapper"], 0)),
          ("loc_enable_from_map: wrong kind of handle", "mapper", lambda S: S["mapper"].loc_enable_from_map(S["mapper"], 0)),
          ("loc_enable_from_map: after the first scan", "used", lambda S: S["used"].loc_enable_from_map(S["mapper"], 0)),
          ("loc_enable_from_map: the mapping handle null", "plain", lambda S: S["plain"].loc_enable_from_map(None, 0)),
          ("loc_enable_from_map: the mapping handle is the handle", "plain", lambda S: S["plain"].loc_enable_from_map(S["plain"], 0)),
          ("loc_enable_from_map: a mapping handle without archive", "plain", lambda S: S["plain"].loc_enable_from_map(S["used"], 0)),
          ("loc_enable_from_map: slot -1 of the mapping handle", "plain", lambda S: S["plain"].loc_enable_from_map(S["mapper"], -1)),
          ("loc_enable_from_map: slot n_slots of the mapping handle", "plain", lambda S: S["plain"].loc_enable_from_map(S["mapper"], N_MAP)),
          ("loc_update_from_map: wrong kind of handle", "plain", lambda S: S["plain"].loc_update_from_map(S["mapper"], 0)),
          ("loc_update_from_map: slot n_slots of the mapping handle", "localiser", lambda S: S["localiser"].loc_update_from_map(S["mapper"], N_MAP)),
          ("reloc_enable: feature off", "plain", lambda S: S["plain"].reloc_enable()),
          ("reloc_enable: wrong kind of handle", "mapper", lambda S: S["mapper"].reloc_enable()),
          ("reloc_enable: a second call", "localiser", lambda S: S["localiser"].reloc_enable()),
          ("trajectory_enable: after alego_stream_setup", "stream", lambda S: S["stream"].trajectory_enable(4)),
          ("trajectory_enable: capacity 0", "plain", lambda S: S["plain"].trajectory_enable(0)),
          ("stream_setup: wrong kind of handle", "localiser", lambda S: S["localiser"].stream_setup(0))]
    return C


def answer(S, scene, call):
    """(code, text) of one case; 0 and "" for a call that is accepted"""
    try:
        S[scene].set_option("api_refusals", 0)   # a refusal with a known text: a case that leaves it in place has set none of its own
    except binding.AlegoError:
        pass
    try:
        call(S)
        return 0, ""
    except binding.AlegoError as e:
        m = re.search(r"failed \((-?\d+)\): (.*)$", str(e), re.S)
        return int(m.group(1)), ("-" if m.group(2) == SENTINEL else m.group(2))


def main():
    S = build_scenes()
    try:
        for name, scene, call in cases():
            code, text = answer(S, scene, call)
            print(f"{name} | {code} | {text}", flush=True)
    finally:
        close_scenes(S)


if __name__ == "__main__":
    main()
