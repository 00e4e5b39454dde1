"""A slot moved by a rigid transform and one slot's key-frame archive merged into another's, on the device (alego_map_move / alego_map_merge,
kernels_merge.hip / merge_math.h).

Both calls are DEFINED by sequences of calls that existed before them (include/alego_mi355x.h).  Every device comparison here is made against
a replica slot of the same handle that is built by that defining host sequence (host_merge / host_move below), byte for byte over every public
getter - with one allowance: the moved poses come from the device's sin / cos / atan2 there and from the host's in alego_map_align_poses, so a
component may differ in its last f32 bit.  The poses are therefore compared first (equal or one f32 ulp apart, at most 1 % unequal), and the
replica is then built with the poses read back from the device result.

The share of unequal components is printed by every test that moves poses (-s).  Measured on the MI355X: 0 of 618 (shapes), 36, 150 (70 pairs),
36 (graph off), 144 (moves) and 138 (the lap) components differ.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from alego_amd import binding, synth
from test_loop_appearance import MAX_RANGE, Z_OFFSET, _sparse, cloud_of, split3
from test_loop_search import LAP, _params, _scan, constraint_reference
from test_map_align import full, gap, inv, rigid, rzryrx_np, truth
from test_relocalize import ANG_TOL, POS_TOL
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ["alego_map_move", "alego_map_merge", "alego_map_align_edge", "alego_map_merge_edges"]
EMPTY = np.zeros((0, 4), F32)
ITEM = binding.MERGE_COPY_ITEM
ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
KINDS = (binding.MAP_SURF, binding.MAP_CORNER, binding.MAP_OUTLIER, ALL, ALL | binding.MAP_FRAME_ID)
K = 4                       # recent_keyframe_num of the constructed handles: the ring holds K + 1 frames
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6])
SEAM = np.array([1e-2, 1e-2, 1e-2, 0.25, 0.25, 0.25])   # a loose seam


# ---- the arithmetic in plain Python floats (IEEE f64, no contraction), every sum in merge_math.h's / pg_math.h's order -------------------
def compose_py(A, B):
    """pg_compose: A B for row-major 3x4 [R | t]"""
    A, B = [float(v) for v in np.asarray(A, np.float64).reshape(12)], [float(v) for v in np.asarray(B, np.float64).reshape(12)]
    out = [0.0] * 12
    for r in range(3):
        for c in range(4):
            out[r * 4 + c] = (A[r * 4 + 0] * B[0 + c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c]
        out[r * 4 + 3] += A[r * 4 + 3]
    return np.array(out).reshape(3, 4)


def between_np(A, B):
    A, B = full(A), full(B)
    return (inv(A) @ B)[:3]


def ulps(a, b):
    """distance of two f32 arrays in units in the last place (sign-magnitude order)"""
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return np.abs(key(a) - key(b))


def check_poses(got, want, tag):
    """every component equal or one f32 ulp apart; at most 1 % unequal; returns (unequal, total)"""
    d = ulps(got, want)
    bad, tot = int((d != 0).sum()), int(d.size)
    print(f"  {tag}: {bad} of {tot} pose components differ from alego_map_align_poses (largest {int(d.max()) if tot else 0} ulp)")
    assert tot == 0 or (d.max() <= 1 and bad <= 0.01 * tot), (tag, bad, tot, int(d.max()))
    return bad, tot


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_merge_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in binding.EXPORTS, s
    for t in ("alego_map_merge_opts", "alego_map_merge_result", "Out of scope", "LOOSE seam"):
        assert t in hdr, t
    assert int(re.search(r"#define ALEGO_MERGE_COPY_ITEM (\d+)", hdr).group(1)) == ITEM
    assert "not part of this interface" not in hdr


def _edges(rng, frm, to):
    n = len(frm)
    return dict(frm=np.asarray(frm, np.int64), to=np.asarray(to, np.int64), between=np.array([rigid(rng.uniform(-0.3, 0.3, 3), rng.uniform(-3, 3, 3))[:3] for _ in range(n)]).reshape(n, 3, 4),
                variance=rng.uniform(1e-8, 1e-2, (n, 6)))


@pytest.mark.parametrize("nd", [0, 1, 5, 1000])
def test_merge_edges_twin_equals_numpy(nd):
    """alego_map_merge_edges: id shifts, variances and order exact; the seam's measurement against numpy with the tolerance test_map_align.py uses
    for alego_map_align_poses against numpy (positions 1e-5 of the largest coordinate, rotations 1e-6)"""
    rng = np.random.default_rng(5 + nd)
    for ns, nl in ((1, 0), (2, 1), (7, 3), (40, 9)):
        ch = _edges(rng, np.arange(ns) - 1, np.arange(ns))
        a, b = rng.integers(0, ns, nl), rng.integers(0, ns, nl)
        lp = _edges(rng, a, b)
        prev = np.r_[rng.uniform(-50, 50, 3), rng.uniform(-0.1, 0.1, 2), rng.uniform(-3, 3)].astype(F32)
        first = np.r_[rng.uniform(-50, 50, 3), rng.uniform(-0.1, 0.1, 2), rng.uniform(-3, 3)].astype(F32)
        oc, ol = binding.map_merge_edges(ch, lp, nd, prev if nd else None, first, SEAM)
        assert oc["frm"].tolist() == (np.arange(ns) - 1 + nd).tolist() and oc["to"].tolist() == (np.arange(ns) + nd).tolist()
        assert_bit_equal(oc["between"][1:], ch["between"][1:], "shifted chain: a measurement stays what was measured")
        assert_bit_equal(oc["variance"][1:], ch["variance"][1:], "shifted chain: variances")
        assert_bit_equal(oc["variance"][0], SEAM, "the seam's variances")
        want = rzryrx_np(first)[:3] if nd == 0 else between_np(rzryrx_np(prev), rzryrx_np(first))
        assert np.abs(oc["between"][0][:, :3] - want[:, :3]).max() < 1e-6 and np.abs(oc["between"][0][:, 3] - want[:, 3]).max() < 1e-5 * max(1.0, np.abs(want[:, 3]).max()), (nd, ns)
        assert ol["frm"].tolist() == (a + nd).tolist() and ol["to"].tolist() == (b + nd).tolist(), "loop edges: ids raised by nd, in their order"
        assert_bit_equal(ol["between"], lp["between"], "loop edges: measurements")
        assert_bit_equal(ol["variance"], lp["variance"], "loop edges: variances")
    L = binding.lib()
    e = binding.graph_edges([-1], [0], [np.eye(4)[:3]], [SEAM])
    assert L.alego_map_merge_edges(e, -1, e, 0, 0, None, None, None, e, e) == binding.ERR_ARG
    assert L.alego_map_merge_edges(None, 1, e, 0, 0, None, None, None, e, e) == binding.ERR_ARG
    assert L.alego_map_merge_edges(e, 0, e, 0, 3, None, None, None, None, None) == 0, "nothing to do"


def _hyp(rng, src_frame, dst_frame, accepted=1, inlier=1, fitness=0.0123):
    guess = np.r_[rng.uniform(-30, 30, 3), rng.uniform(-0.1, 0.1, 2), rng.uniform(-3, 3)].astype(F32)
    icp = rigid(rng.uniform(-0.05, 0.05, 3), rng.uniform(-1, 1, 3)).astype(F32)
    return dict(src_frame=src_frame, dst_frame=dst_frame, dist=7, shift=3, tried=1, accepted=accepted, converged=1, iterations=9, n_source=100, n_target=900,
                support=2, inlier=inlier, fitness=fitness, guess6=guess, icp_final=icp, T=np.eye(4, dtype=F32))


def test_align_edge_twin_equals_numpy():
    """alego_map_align_edge: ids and variances exact, the measurement against tests/test_loop_search.py's restatement of alego_loop_constraint"""
    rng = np.random.default_rng(17)
    for nd in (0, 1, 5, 300):
        x = _hyp(rng, 11, 4, fitness=float(rng.uniform(1e-3, 0.2)))
        dst6 = np.r_[rng.uniform(-30, 30, 3), rng.uniform(-0.1, 0.1, 2), rng.uniform(-3, 3)].astype(F32)
        e = binding.map_align_edge(x, dst6, nd)
        assert (e["frm"], e["to"]) == (nd + 11, 4)
        assert_bit_equal(e["variance"], np.full(6, float(F32(x["fitness"]))), "all six variances are (float)fitness")
        _, want = constraint_reference(x["icp_final"], x["guess6"], dst6)
        assert np.abs(e["between"] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (nd, e["between"], want)
        assert_bit_equal(e["between"], binding.loop_constraint(x["icp_final"], x["guess6"], dst6)[1], "the library's own alego_loop_constraint")
    for bad in (_hyp(rng, 1, 2, accepted=0), _hyp(rng, 1, 2, inlier=0)):
        with pytest.raises(binding.AlegoError):
            binding.map_align_edge(bad, np.zeros(6, F32), 3)


def test_merge_math_stand_alone(tmp_path):
    """tests/merge_math/merge_math_check.cpp over csrc/merge_math.h, built with AddressSanitizer and UBSan as a program of its own"""
    exe = str(tmp_path / "merge_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "merge_math", "merge_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "merge_math ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


# ---- GPU: the replica, the snapshot ------------------------------------------------------------------------------------------
def graph_on(h):
    try:
        h.graph_status(0)
        return True
    except binding.AlegoError:
        return False


def snap(h, s, k=K):
    """everything the public getters say about slot s, as (name, array) pairs"""
    out = []
    st = h.map_status(s)
    out.append(("map_status", np.array(st)))
    for j in range(st[0]):
        f = h.map_get_keyframe(j, slot=s)
        out += [(f"archived frame {j}: {key}", f[key]) for key in ("pose", "corner", "surf", "outlier")]
    out += [(f"map_assemble kinds {kinds}", h.map_assemble(kinds, slot=s)) for kinds in KINDS]
    out.append(("stamps", h.map_get_stamps(slot=s)))
    nk = h.lm_keyframe_count(slot=s)
    out.append(("lm_keyframe_count", np.array(nk)))
    for j in range(max(0, nk - k), nk):
        f = h.lm_get_keyframe(j, slot=s)
        out += [(f"resident frame {j}: {key}", f[key]) for key in ("pose", "corner", "surf", "outlier")]
    out += [(name, h.debug_get(name, slot=s)) for name in ("lm_state", "lm_info", "lm_kf_corner_map", "lm_kf_surf_map")]
    if graph_on(h):
        gs = h.graph_status(s)
        out.append(("graph_status", np.array(gs)))
        for kind, what in ((0, "chain"), (1, "loop")):
            e = h.graph_get_edges(kind=kind, slot=s)
            out += [(f"{what} edges: {key}", e[key]) for key in ("frm", "to", "between", "variance")]
        out.append(("the graph's estimate", h.graph_get_estimate(n=gs[3], slot=s)))
    return out


def same(a, b, tag):
    assert [n for n, _ in a] == [n for n, _ in b], (tag, len(a), len(b))
    for (name, x), (_, y) in zip(a, b):
        assert_bit_equal(np.asarray(x), np.asarray(y), f"{tag}: {name}")


def archived_poses(h, s):
    return np.array([h.map_get_keyframe(j, slot=s)["pose"] for j in range(h.map_status(s)[0])], F32).reshape(-1, 6)


def host_merge(h, src, dst, poses, stamp_offset=0.0, seam_variance=None, hyp=None):
    """the DEFINING host sequence of alego_map_merge for one pair, with the moved poses given"""
    ns, nd = h.map_status(src)[0], h.map_status(dst)[0]
    if ns == 0:
        return
    graph = graph_on(h)
    frames = [h.map_get_keyframe(f, slot=src) for f in range(ns)]
    stamps = h.map_get_stamps(slot=src)
    dst_poses = archived_poses(h, dst)
    h.lm_reset_window(slot=dst)
    for f in range(ns):
        h.lm_add_keyframe(poses[f], frames[f]["corner"], frames[f]["surf"], frames[f]["outlier"], slot=dst)
    h.map_set_stamps(nd, stamps + stamp_offset, slot=dst)
    if not graph:
        return
    ch, lp = h.graph_get_edges(kind=0, slot=src), h.graph_get_edges(kind=1, slot=src)
    if ns > 1:
        h.graph_set_edges(nd + 1, ch["frm"][1:] + nd, ch["to"][1:] + nd, ch["between"][1:], ch["variance"][1:], slot=dst)
    seam = h.graph_get_edges(kind=0, first=nd, n=1, slot=dst)   # as the archive recorded it; only its variances are the caller's
    h.graph_set_edges(nd, seam["frm"], seam["to"], seam["between"], [ODOM_VAR if seam_variance is None else seam_variance], slot=dst)
    for i in range(len(lp["frm"])):
        h.graph_add_edge(int(lp["frm"][i]) + nd, int(lp["to"][i]) + nd, lp["between"][i], lp["variance"][i], slot=dst)
    for x in hyp or []:
        if x["accepted"] and x["inlier"]:
            e = binding.map_align_edge(x, dst_poses[x["dst_frame"]], nd)
            h.graph_add_edge(e["frm"], e["to"], e["between"], e["variance"], slot=dst)


def host_move(h, s, poses, T, k=K):
    """the DEFINING host sequence of alego_map_move for one slot, with the moved poses given"""
    n = h.map_status(s)[0]
    h.map_set_keyposes(0, poses, slot=s)
    for kf in range(max(0, n - k), n):
        h.lm_set_keypose(kf, poses[kf], slot=s)
    h.lm_reset_window(slot=s)
    h.lm_apply_correction(np.asarray(T, np.float64)[:3].reshape(12), slot=s)
    if graph_on(h):
        e = h.graph_get_edges(kind=0, first=0, n=1, slot=s)
        h.graph_set_edges(0, [-1], [0], [compose_py(np.asarray(T, np.float64)[:3], e["between"][0])], e["variance"], slot=s)


def rigid64(rpy, t):
    """a rigid 3x4 whose rotation is orthonormal to f64 rounding (test_map_align.rigid's comes from f32 arithmetic: R^T is its inverse to 1e-7 only)"""
    import pose_graph_ref as R
    return np.c_[R.rzryrx(*[float(v) for v in rpy]), np.asarray(t, np.float64).reshape(3, 1)]


def rand_poses(rng, n):
    return np.c_[rng.uniform(-30, 30, (n, 3)), rng.uniform(-0.05, 0.05, (n, 2)), rng.uniform(-3, 3, (n, 1))].astype(F32)


def rand_clouds(rng, n, pts=None):
    """n constructed clouds (one point per non-zero descriptor bin); pts: cut every cloud to that many points"""
    out = [cloud_of(D) for D in _sparse(rng, n)]
    return out if pts is None else [c[:pts] for c in out]


def add(h, s, clouds, poses, stamps=None):
    for c, pose in zip(clouds, poses):
        if isinstance(c, tuple):
            h.lm_add_keyframe(pose, *c, slot=s)
        else:
            h.lm_add_keyframe(pose, *split3(np.ascontiguousarray(c, F32).reshape(-1, 4)), slot=s)
    if stamps is not None:
        h.map_set_stamps(0, stamps, slot=s)


def add_loops(h, s, rng, n):
    nf = h.map_status(s)[0]
    for _ in range(n):
        a, b = rng.choice(nf, 2, replace=False)
        h.graph_add_edge(int(a), int(b), rigid(rng.uniform(-0.1, 0.1, 3), rng.uniform(-2, 2, 3))[:3], rng.uniform(1e-4, 1e-2, 6), slot=s)


def merge_and_compare(h, pairs, replicas, T, tag, stamp_offset=0.0, seam_variance=None, hyps=None, optimise=True):
    """device merge of `pairs`, pose check against alego_map_align_poses, the host sequence on the replicas with the device's poses, snapshots equal"""
    srcs = sorted({s for s, _ in pairs})
    before = {s: snap(h, s) for s in srcs}
    src_poses = {s: archived_poses(h, s) for s in srcs}
    nd = {d: h.map_status(d)[0] for _, d in pairs}
    res = h.map_merge(pairs, T, stamp_offset=stamp_offset, seam_variance=seam_variance, hyps=hyps)
    Ts = [np.asarray(T, np.float64)] * len(pairs) if np.asarray(T).ndim == 2 else list(np.asarray(T, np.float64))
    bad = tot = 0
    for i, ((s, d), r) in enumerate(zip(pairs, res)):
        ns = len(src_poses[s])
        assert (r["status"], r["frames"]) == ((2, ns) if ns else (0, 0)), (tag, s, d, r)
        got = archived_poses(h, d)[nd[d]:]
        want = binding.map_align_poses(Ts[i][:3], src_poses[s])
        d_ = ulps(got, want)
        assert d_.size == 0 or d_.max() <= 1, (tag, s, d, int(d_.max()))
        bad, tot = bad + int((d_ != 0).sum()), tot + int(d_.size)
        host_merge(h, s, replicas[i], got, stamp_offset, seam_variance, hyps[i] if hyps else None)
    print(f"  {tag}: {bad} of {tot} moved pose components differ from alego_map_align_poses")
    assert bad <= 0.01 * tot, (tag, bad, tot)
    for i, (s, d) in enumerate(pairs):
        same(snap(h, d), snap(h, replicas[i]), f"{tag}: dst {d} against its replica {replicas[i]} (source {s})")
    for s in srcs:
        same(before[s], snap(h, s), f"{tag}: the source slot {s} before and after")
    if optimise and graph_on(h):
        ds, rs = [d for _, d in pairs], list(dict.fromkeys(replicas))
        ga, gb = h.graph_optimize(ds), h.graph_optimize(rs)
        for i, (s, d) in enumerate(pairs):
            a, b = ga[i], gb[rs.index(replicas[i])]
            for key in a:
                assert_bit_equal(np.asarray(a[key]), np.asarray(b[key]), f"{tag}: optimise of dst {d}: {key}")
            n = h.graph_status(d)[3]
            assert_bit_equal(h.graph_get_estimate(n=n, slot=d), h.graph_get_estimate(n=n, slot=replicas[i]), f"{tag}: estimate of dst {d}")
    return res, bad, tot


NS_CASES = (1, K, K + 1, K + 2, 2 * K + 3)
ND_CASES = (0, 1, 5)


@pytest.fixture(scope="module")
def shapes():
    """one 128-slot handle (two stream groups of 64), K = 4, graph on.  Slots 0 .. 4: sources of NS_CASES frames; slot 5: a source of three copy
    items plus an odd remainder with an empty corner / surf / outlier cloud and a frame with no point at all; destinations from slot 56 on, so
    that they span both stream groups; replicas from slot 96 on"""
    rng = np.random.default_rng(41)
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=128)
    assert h.stream_groups()[1] == 64
    h.map_enable(40, 1 << 14)
    h.graph_enable(8, ODOM_VAR)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    for s, ns in enumerate(NS_CASES):
        add(h, s, rand_clouds(rng, ns, 90), rand_poses(rng, ns), stamps=np.arange(ns) * 7.5 + s)
        if ns >= 3:
            add_loops(h, s, rng, 2)
    tot = 3 * ITEM + 37
    pool = [split3(c) for c in rand_clouds(rng, 16)]
    pool[1] = (EMPTY, pool[1][1], pool[1][2])
    pool[2] = (pool[2][0], EMPTY, pool[2][2])
    pool[3] = (pool[3][0], pool[3][1], EMPTY)
    pool[4] = (EMPTY, EMPTY, EMPTY)
    frames, have = [], 0
    for f in pool:   # whole frames while they fit, then one cut to the remainder
        n = sum(len(x) for x in f)
        if have + n >= tot:
            frames.append(split3(np.concatenate(f)[:tot - have]))
            have = tot
            break
        frames.append(f)
        have += n
    assert have == tot and 6 <= len(frames) <= 16, (have, len(frames))
    add(h, 5, frames, rand_poses(rng, len(frames)), stamps=np.arange(len(frames)) * 3.0)
    assert h.map_status(5)[2] == tot and tot % ITEM == 37
    add_loops(h, 5, rng, 3)
    yield dict(h=h, rng=rng)
    h.close()


def _dst_pairs(h, rng, sources, first_dst, first_rep, nds=ND_CASES):
    """for every (source, nd): a destination and its replica with the same nd frames and one loop edge where nd allows it"""
    pairs, reps = [], []
    d, r = first_dst, first_rep
    for s in sources:
        for nd in nds:
            cl, po = rand_clouds(rng, nd, 60), rand_poses(rng, nd)
            lp_seed = int(rng.integers(1 << 30))
            for slot in (d, r):
                add(h, slot, cl, po, stamps=np.arange(nd) * 2.0)
                if nd >= 2:
                    add_loops(h, slot, np.random.default_rng(lp_seed), 1)
            pairs.append((s, d)); reps.append(r)
            d, r = d + 1, r + 1
    return pairs, reps


@pytest.mark.gpu
def test_merge_equals_the_host_sequence_for_every_shape(shapes):
    """ns in {1, K, K + 1, K + 2, 2 K + 3} x nd in {0, 1, 5} in ONE call: every source feeds three destinations, the destinations lie in both
    stream groups; the big source (three copy items + 37 points, empty clouds, an empty frame) goes into an empty and a non-empty destination"""
    h, rng = shapes["h"], shapes["rng"]
    pairs, reps = _dst_pairs(h, rng, list(range(len(NS_CASES))), 56, 96)
    more, mreps = _dst_pairs(h, rng, [5], 56 + len(pairs), 96 + len(pairs), nds=(0, 5))
    pairs, reps = pairs + more, reps + mreps
    assert min(d for _, d in pairs) < 64 <= max(d for _, d in pairs), "both stream groups"
    T = np.array([rigid(rng.uniform(-0.03, 0.03, 3) * [1, 1, 30], rng.uniform(-40, 40, 3))[:3] for _ in pairs])
    res, bad, tot = merge_and_compare(h, pairs, reps, T, "shapes", stamp_offset=1000.25, seam_variance=SEAM)
    assert [r["loop_edges"] for r in res] == [0] * 3 + [2] * 12 + [3] * 2, [r["loop_edges"] for r in res]
    assert res[-1]["points"] == 3 * ITEM + 37 and all(r["cross_edges"] == 0 for r in res)
    shapes["merged"] = (pairs, reps)


@pytest.mark.gpu
def test_a_second_merge_and_the_lazy_descriptors(shapes):
    """a destination that was merged into takes another source (its newest frames are source frames now, its seam follows a moved pose), with
    the default seam variance and no stamp offset; the appearance search then describes the appended frames as on the host-merged replica"""
    h, rng = shapes["h"], shapes["rng"]
    pairs, reps = shapes["merged"]
    i = 1 * len(ND_CASES) + 2                      # source 1 (K frames) into nd = 5: 5 + K frames so far
    assert pairs[i][0] == 1 and h.map_status(pairs[i][1])[0] == 5 + K
    d, r = pairs[i][1], reps[i]
    T = rigid([0.0, 0.01, -2.0], [5, 6, 0.5])[:3]
    merge_and_compare(h, [(3, d)], [r], T, "a second merge")
    x, y = h.loop_search_appearance([d, r], verify=0)
    for key in sorted(x):
        assert_bit_equal(np.asarray(x[key]), np.asarray(y[key]), f"appearance search on the merged destination and its replica: {key}")
    assert_bit_equal(h.debug_get("la_desc", slot=d), h.debug_get("la_desc", slot=r), "descriptors of the union")
    assert h.debug_get("la_desc", slot=d).size == 1200 * h.map_status(d)[0]


@pytest.mark.gpu
def test_seventy_pairs_in_one_call():
    """70 pairs on a 128-slot handle: 7 configurations (source, nd) x 10 destinations each in slots 20 .. 89, which span both stream groups;
    every destination against the replica of its configuration; the slots that are not in the call are byte-equal around it"""
    rng = np.random.default_rng(43)
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=128)
    h.map_enable(16, 1 << 12)
    h.graph_enable(4, ODOM_VAR)
    try:
        cfg = [(0, 0), (0, 2), (1, 0), (1, 1), (2, 3), (2, 0), (1, 6)]   # (source, nd)
        for s, ns in enumerate((1, 3, 7)):
            add(h, s, rand_clouds(rng, ns, 45), rand_poses(rng, ns))
        add_loops(h, 2, rng, 2)
        setups = [(rand_clouds(rng, nd, 30), rand_poses(rng, nd)) for _, nd in cfg]
        pairs, reps, Ts = [], [], []
        T7 = [rigid(rng.uniform(-0.02, 0.02, 3) * [1, 1, 50], rng.uniform(-20, 20, 3))[:3] for _ in cfg]
        for c, (s, nd) in enumerate(cfg):
            add(h, 100 + c, *setups[c])
        for j in range(70):
            c = j % 7
            add(h, 20 + j, *setups[c])
            pairs.append((cfg[c][0], 20 + j)); reps.append(100 + c); Ts.append(T7[c])
        add(h, 10, rand_clouds(rng, 3, 30), rand_poses(rng, 3))     # bystanders in both groups
        add(h, 95, rand_clouds(rng, 6, 30), rand_poses(rng, 6))
        by = {s: snap(h, s) for s in (10, 95, 3, 127)}
        # the replicas are built once per configuration: the host sequence runs on the first pair of each, later pairs only compare
        srcs = {s: archived_poses(h, s) for s in range(3)}
        res = h.map_merge(pairs, np.array(Ts), seam_variance=SEAM)
        assert [r["status"] for r in res] == [2] * 70
        bad = tot = 0
        for c, (s, nd) in enumerate(cfg):
            got = archived_poses(h, 20 + c)[nd:]
            d_ = ulps(got, binding.map_align_poses(T7[c], srcs[s]))
            assert d_.max() <= 1
            bad, tot = bad + int((d_ != 0).sum()), tot + int(d_.size)
            host_merge(h, s, 100 + c, got, 0.0, SEAM)
        print(f"  70 pairs: {bad} of {tot} moved pose components differ from alego_map_align_poses")
        assert bad <= 0.01 * tot
        want = [snap(h, 100 + c) for c in range(7)]
        for j, (s, d) in enumerate(pairs):
            same(snap(h, d), want[j % 7], f"70 pairs: dst {d} against the replica of configuration {j % 7}")
        for s, b in by.items():
            same(b, snap(h, s), f"70 pairs: bystander slot {s}")
    finally:
        h.close()


@pytest.mark.gpu
def test_merge_with_the_graph_off():
    rng = np.random.default_rng(47)
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=4)
    h.map_enable(16, 1 << 12)
    try:
        add(h, 0, rand_clouds(rng, K + 2, 40), rand_poses(rng, K + 2), stamps=np.arange(K + 2) * 1.5)
        cl, po = rand_clouds(rng, 2, 40), rand_poses(rng, 2)
        add(h, 1, cl, po); add(h, 2, cl, po)
        x = _hyp(rng, 1, 0)
        res, _, _ = merge_and_compare(h, [(0, 1)], [2], rigid([0, 0, 1.0], [1, 2, 3])[:3], "graph off", seam_variance=SEAM, hyps=[[x]])
        assert res[0] == dict(status=2, frames=K + 2, points=h.map_status(0)[2], loop_edges=0, cross_edges=0), res
    finally:
        h.close()


@pytest.mark.gpu
def test_fit_edges_and_errors():
    """frames, points and loop edges each exactly at capacity give 2, one over gives -3 with dst byte-unchanged while the other pairs of the call
    merge; dropped frames give -1, an empty source 0; every ALEGO_ERR_ARG case leaves all slots untouched"""
    rng = np.random.default_rng(53)
    MAXF, MAXP, MAXL = 8, 600, 3
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=16)
    h.map_enable(MAXF, MAXP)
    h.graph_enable(MAXL, ODOM_VAR)
    try:
        # sources: slot 0: 3 frames x 60 points, 1 loop edge; slot 1: 3 frames x 100 points; slot 2: empty; slot 3: dropped frames
        add(h, 0, rand_clouds(rng, 3, 60), rand_poses(rng, 3)); add_loops(h, 0, rng, 1)
        add(h, 1, rand_clouds(rng, 3, 100), rand_poses(rng, 3))
        for s in (3, 15):
            add(h, s, rand_clouds(rng, MAXF + 1, 30), rand_poses(rng, MAXF + 1))
            assert h.map_status(s)[1] == 1
        def dst(slots, nd, pts, loops):
            cl, po, seed = rand_clouds(rng, nd, pts), rand_poses(rng, nd), int(rng.integers(1 << 30))
            for s in slots:
                add(h, s, cl, po)
                if loops:
                    add_loops(h, s, np.random.default_rng(seed), loops)
        dst((4, 5), MAXF - 3, 30, 0)      # frames exactly at capacity with a source of 3
        dst((6,), MAXF - 2, 30, 0)        # one frame over
        dst((7, 8), 3, 100, 0)            # points: 300 + 300 = MAXP exactly with source 1
        dst((9,), 3, 101, 0)              # one point over (303 + 300)
        dst((10, 11), 3, 30, 2)           # loops: 2 + 1 = MAXL exactly with source 0
        dst((12,), 3, 30, 3)              # one loop edge over
        x = _hyp(rng, 1, 0)
        T = rigid([0, 0, 0.3], [3, 2, 1])[:3]
        unchanged = {s: snap(h, s) for s in (6, 9, 12, 13, 14, 3, 15)}
        pairs = [(0, 4), (0, 6), (1, 7), (1, 9), (0, 10), (0, 12), (2, 13), (3, 14), (0, 15)]
        res = h.map_merge(pairs, T, seam_variance=SEAM)
        assert [r["status"] for r in res] == [2, -3, 2, -3, 2, -3, 0, -1, -1], [r["status"] for r in res]
        for s, b in unchanged.items():
            same(b, snap(h, s), f"fit edges: slot {s} of a pair that did not merge")
        for (s, d), rep in (((0, 4), 5), ((1, 7), 8), ((0, 10), 11)):
            host_merge(h, s, rep, archived_poses(h, d)[h.map_status(rep)[0]:], 0.0, SEAM)
            same(snap(h, d), snap(h, rep), f"fit edges: dst {d} at capacity")
        assert h.map_status(4)[0] == MAXF and h.map_status(7)[2] == MAXP and h.graph_status(10)[1] == MAXL
        # an inlier edge counts against max_loops: slot 13 (empty) takes source 0 (1 loop) + 2 hypotheses = MAXL; + 3 is one over
        hy = lambda n: [[_hyp(rng, 1, 0) for _ in range(n)]]
        add(h, 13, rand_clouds(rng, 1, 30), rand_poses(rng, 1))
        b13 = snap(h, 13)
        assert h.map_merge([(0, 13)], T, hyps=hy(3))[0]["status"] == -3
        same(b13, snap(h, 13), "one cross edge over max_loops")
        r = h.map_merge([(0, 13)], T, hyps=hy(2))[0]
        assert (r["status"], r["loop_edges"], r["cross_edges"]) == (2, 1, 2) and h.graph_status(13)[1] == MAXL, r
        # ---- ALEGO_ERR_ARG: nothing is touched
        every = {s: snap(h, s) for s in range(16)}
        bad_T = T.copy(); bad_T[1, 2] = np.nan
        inf_T = T.copy(); inf_T[0, 3] = np.inf
        cases = [dict(pairs=[(0, 16)]), dict(pairs=[(-1, 1)]), dict(pairs=[(5, 5)]), dict(pairs=[(0, 5), (1, 5)]), dict(pairs=[(0, 5), (5, 8)]), dict(pairs=[(5, 8), (0, 5)]),
                 dict(pairs=[(0, 5)], T=bad_T), dict(pairs=[(0, 5)], T=inf_T), dict(pairs=[(0, 5)], seam_variance=[1, 1, 1, 0, 1, 1]),
                 dict(pairs=[(0, 5)], seam_variance=[1, 1, -1, 1, 1, 1]), dict(pairs=[(0, 5)], seam_variance=[1, np.inf, 1, 1, 1, 1]),
                 dict(pairs=[(0, 5)], stamp_offset=np.nan),
                 # (a pair that fits, slot 9 with 3 frames: a pair that does not fit is -3 before its hypotheses are looked at)
                 dict(pairs=[(0, 9)], hyps=[[_hyp(rng, 3, 0)]]), dict(pairs=[(0, 9)], hyps=[[_hyp(rng, 0, 5)]]),
                 dict(pairs=[(0, 9)], hyps=[[_hyp(rng, 0, 0, fitness=0.0)]]), dict(pairs=[(0, 9)], hyps=[[_hyp(rng, 0, 0, fitness=float("nan"))]])]
        for c in cases:
            kw = dict(c)
            with pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_ARG}\)"):
                h.map_merge(kw.pop("pairs"), kw.pop("T", T), **kw)
        for c in (dict(slots=[16]), dict(slots=[0, 1, 0]), dict(slots=[0], T=bad_T), dict(slots=[-1])):
            with pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_ARG}\)"):
                h.map_move(c["slots"], c.get("T", T))
        for s, b in every.items():
            same(b, snap(h, s), f"ALEGO_ERR_ARG: slot {s}")
        assert h.map_merge([], T) == [] and h.map_move([], T) == []
        assert h.map_move([2, 3, 14], T) == [0, -1, 0], "no key frame / dropped frames"
        for s in (2, 3, 14):
            same(every[s], snap(h, s), f"a move with status != 2: slot {s}")
    finally:
        h.close()
    # the archive off, a localising handle
    h = binding.Handle(_params(False), n_slots=2)
    try:
        for call in (lambda: h.map_merge([(0, 1)], T), lambda: h.map_move([0], T)):
            with pytest.raises(binding.AlegoError, match="the key-frame archive is off"):
                call()
        h.loc_enable([(np.zeros(6, F32), EMPTY, EMPTY, EMPTY)], 0.0)
        for call in (lambda: h.map_merge([(0, 1)], T), lambda: h.map_move([0], T)):
            with pytest.raises(binding.AlegoError, match="not available on a localising handle"):
                call()
    finally:
        h.close()


# ---- alego_map_move ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_move_equals_the_host_sequence_and_survives_an_optimise():
    """slots of 1, K - 1, K, K + 1 and 2 K + 3 frames in both stream groups moved in one call, each against its replica; an optimise afterwards
    leaves the poses moved - with a chain only the estimate equals the moved poses to the margins tests/test_pose_graph.py asserts; moving by
    G and then by G^-1 returns every pose within one f32 ulp per step, the ulp taken at the largest magnitude the component has on the way
    (a position's rounding error of step one is carried through step two at that magnitude; an angle's at pi)"""
    from test_pose_graph import TOL_R, TOL_T, _estimate_error
    import pose_graph_ref as R
    rng = np.random.default_rng(59)
    h = binding.Handle(_params(False, recent_keyframe_num=K), n_slots=128)
    h.map_enable(16, 1 << 12)
    h.graph_enable(4, ODOM_VAR)
    try:
        sizes = (1, K - 1, K, K + 1, 2 * K + 3)
        dev, rep = [3, 20, 63, 64, 90], [4, 21, 62, 65, 91]
        for n, a, b in zip(sizes, dev, rep):
            cl, po = rand_clouds(rng, n, 50), rand_poses(rng, n)
            add(h, a, cl, po); add(h, b, cl, po)
        X = R.from_pose6(po)              # one slot with a loop edge (what its poses say, slightly off) and an estimate
        meas = R.compose(R.between(X[2 * K + 2], X[0]), rigid([0, 0, 0.01], [0.05, 0.02, 0])[:3])
        for s in (dev[4], rep[4]):
            h.graph_add_edge(2 * K + 2, 0, meas, np.full(6, 1e-2), slot=s)
            assert h.graph_optimize([s])[0]["status"] == 2
        add(h, 7, rand_clouds(rng, 3, 50), rand_poses(rng, 3))
        bystander = snap(h, 7)
        G = np.array([rigid64(rng.uniform(-0.02, 0.02, 3) * [1, 1, 60], rng.uniform(-30, 30, 3)) for _ in dev])
        before = [archived_poses(h, s) for s in dev]
        assert h.map_move(dev, G) == [2] * 5
        bad = tot = 0
        for i, (a, b) in enumerate(zip(dev, rep)):
            got = archived_poses(h, a)
            x, y = check_poses(got, binding.map_align_poses(G[i], before[i]), f"move of slot {a}")
            bad, tot = bad + x, tot + y
            host_move(h, b, got, G[i])
            same(snap(h, a), snap(h, b), f"move: slot {a} against its replica {b}")
        assert bad <= 0.01 * tot
        same(bystander, snap(h, 7), "move: a slot that is not in the call")
        # the optimise: chain-only slots stay where the move put them
        ga, gb = h.graph_optimize(dev, apply=True), h.graph_optimize(rep, apply=True)
        for i, (a, b) in enumerate(zip(dev, rep)):
            for key in ga[i]:
                assert_bit_equal(np.asarray(ga[i][key]), np.asarray(gb[i][key]), f"optimise after the move, slot {a}: {key}")
            same(snap(h, a), snap(h, b), f"optimise after the move: slot {a} against its replica")
            if i < 4:   # chain only: the optimum is the f64 image of the poses the chain was measured on, moved (the archived f32 poses are its rounding)
                assert ga[i]["status"] == 2 and ga[i]["cost"] <= ga[i]["cost0"], ga[i]
                dt, dr = _estimate_error(h.graph_get_estimate(slot=a), R.compose(G[i], R.from_pose6(before[i])))
                print(f"  optimise after the move, slot {a}: |dt| {dt:.3e} m |dr| {dr:.3e} rad")
                assert dt <= TOL_T and dr <= TOL_R, (a, dt, dr)
                assert np.abs(archived_poses(h, a)[:, :3] - binding.map_align_poses(G[i], before[i])[:, :3]).max() < 1e-4, "the slot stays moved"
        assert ga[4]["applied"] == 1
        moved = archived_poses(h, dev[4])
        want = binding.map_align_poses(G[4], before[4])
        assert np.abs(moved[:, :3] - want[:, :3]).max() < 0.5 and np.abs(moved[:, :3] - before[4][:, :3]).max() > 5.0, "the optimise with a loop edge keeps the slot moved"
        # G, then G^-1
        s = dev[2]
        p0 = archived_poses(h, s)
        Gi = inv(full(G[2]))[:3]
        assert h.map_move([s], Gi) == [2]
        p1 = archived_poses(h, s)
        orig = before[2]
        mag = np.maximum(np.abs(orig[:, :3]), np.abs(p0[:, :3])).max(axis=1, keepdims=True)
        tol = np.c_[2 * np.spacing(np.broadcast_to(mag, (len(orig), 3)).astype(F32)), np.full((len(orig), 3), 2 * np.spacing(F32(np.pi)))]
        err = np.abs(p1.astype(np.float64) - orig.astype(np.float64))
        err[:, 3:] = np.minimum(err[:, 3:], np.abs(err[:, 3:] - 2 * np.pi))
        print(f"  G then G^-1: largest error / allowance {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (err, tol)
    finally:
        h.close()


# ---- the lap: two sessions become one map ----------------------------------------------------------------------------------------
SRC_SCANS, DST_SCANS, DST_START, MORE = 251, 171, 100, 10


@pytest.mark.gpu
def test_lap_two_sessions_become_one_map():
    """tests/test_map_align.py's set-up: the source is scans 0 - 250 (slot 0), the destination scans 100 - 270 (slot 1, its replica slot 2), so the
    source's newest frames lie where the destination's stream stands.  Align, merge with the hypotheses and a loose seam, optimise with apply = 1,
    run the destination ten more scans: byte for byte the replica.  Both loop searches and an alignment on the union return what they return on the
    replica.

    The union's key poses of the source frames against synth's ground truth.  With (dp, da) the largest distance of an inlier hypothesis' T from
    the truth, as DESIGN.md section 17 measures it (translation column, rotation angle), p the true position of a source frame in the source's
    frame and e its own error there (the drift of the stretch): |T_est p_est - T_true p_true| <= |p_est - p_true| + |T_est p_true - T_true p_true|
    <= e + dp + da |p|.  So the allowance is dp + da max|p| + max e in position and da + the largest angle of the stretch's drift in rotation;
    dp, da come from alego_map_align's output and the drift from the source slot as the host sequence of the replica reads it, none from the
    code under test.  Measured on the MI355X: alignment 0.1472 m / 0.01008 rad, reach 17.2 m, drift 0.0697 m / 0.00628 rad, so the allowance is
    0.3909 m / 0.01636 rad; the union's source frames lie 0.1143 m / 0.01017 rad from the truth."""
    p = _params(False)
    KK = p.recent_keyframe_num
    # (a key frame waits for its sort until the next VoxelGrid round of its stream GROUP, whichever slot's scan starts it: the destination and its replica
    # lie in two groups, so that neither's scans touch the other's pending frame and the scratch words of lm_info agree; the source ran before both)
    D, RP = 1, 65
    h = binding.Handle(p, n_slots=128)
    assert h.stream_groups()[1] == 64
    h.map_enable(128, 1 << 20)
    h.graph_enable(40)
    h.loop_appearance_enable(MAX_RANGE, Z_OFFSET)
    try:
        for k in range(SRC_SCANS):
            h.scan_process(_scan(p, k), stages=7, slot=0, stamp=0.1 * k)
        for k in range(DST_SCANS):
            for s in (D, RP):
                h.scan_process(_scan(p, (DST_START + k) % LAP), stages=7, slot=s, stamp=0.1 * k)
        same(snap(h, D, KK), snap(h, RP, KK), "lap: the destination and its replica before the merge")
        r = h.map_align([(0, D)])[0]
        assert r["status"] == 2, r
        src_poses, nd, ns = archived_poses(h, 0), h.map_status(D)[0], h.map_status(0)[0]
        src_before = snap(h, 0, KK)
        res = h.map_merge([(0, D)], r["T"], seam_variance=SEAM, hyps=[r["hyp"]])[0]
        n_in = sum(1 for x in r["hyp"] if x["accepted"] and x["inlier"])
        assert res == dict(status=2, frames=ns, points=h.map_status(0)[2], loop_edges=0, cross_edges=n_in) and n_in >= 2, (res, n_in)
        got = archived_poses(h, D)[nd:]
        check_poses(got, binding.map_align_poses(r["T"], src_poses), "lap: merged poses")
        host_merge(h, 0, RP, got, 0.0, SEAM, r["hyp"])
        same(snap(h, D, KK), snap(h, RP, KK), "lap: after the merge")
        same(src_before, snap(h, 0, KK), "lap: the source slot before and after")
        ga, gb = h.graph_optimize([D], apply=True)[0], h.graph_optimize([RP], apply=True)[0]
        assert ga["status"] == 2 and ga["applied"] == 1 and ga["n_poses"] == nd + ns and ga["n_loops"] == n_in, ga
        for key in ga:
            assert_bit_equal(np.asarray(ga[key]), np.asarray(gb[key]), f"lap: optimise of the union: {key}")
        same(snap(h, D, KK), snap(h, RP, KK), "lap: after the optimise")
        for k in range(MORE):
            out = [h.scan_process(_scan(p, (DST_START + DST_SCANS + k) % LAP), stages=7, slot=s, stamp=0.1 * (DST_SCANS + k)) for s in (D, RP)]
            assert out[0][0] == out[1][0], (k, out[0][0], out[1][0])
            for a, b, what in ((out[0][1], out[1][1], "odometry"), (out[0][2], out[1][2], "map pose")):
                for key in ("t", "q", "params"):
                    assert_bit_equal(a[key], b[key], f"lap: scan {k} after the merge: {what} {key}")
            assert_bit_equal(h.debug_get("lm_info", slot=D), h.debug_get("lm_info", slot=RP), f"lap: scan {k} after the merge: lm_info")
        same(snap(h, D, KK), snap(h, RP, KK), f"lap: {MORE} scans after the merge")
        # ---- the ground truth
        scans = np.rint(h.map_get_stamps(slot=0) / 0.1).astype(int)
        T_true = truth(DST_START, 0)
        hyp_err = np.array([gap(x["T"], T_true) for x in r["hyp"] if x["accepted"] and x["inlier"]])
        dp, da = hyp_err[:, 0].max(), hyp_err[:, 1].max()
        assert dp < POS_TOL and da < ANG_TOL, (dp, da)
        own = np.array([gap(rzryrx_np(src_poses[f]), truth(0, int(scans[f]))) for f in range(ns)])
        reach = max(np.linalg.norm(truth(0, int(k))[:3, 3]) for k in scans)
        allow_p, allow_a = dp + da * reach + own[:, 0].max(), da + own[:, 1].max()
        for slot, what in ((RP, "the replica"), (D, "the device")):
            union = archived_poses(h, slot)[nd:nd + ns]
            err = np.array([gap(rzryrx_np(union[f]), truth(DST_START, int(scans[f]))) for f in range(ns)])
            print(f"  lap, {what}: source frames of the union {err[:, 0].max():.4f} m / {err[:, 1].max():.5f} rad from the truth; allowance {allow_p:.4f} m / {allow_a:.5f} rad "
                  f"(alignment {dp:.4f} m / {da:.5f} rad over a reach of {reach:.1f} m, drift of the stretch {own[:, 0].max():.4f} m / {own[:, 1].max():.5f} rad)")
            assert err[:, 0].max() <= allow_p and err[:, 1].max() <= allow_a, (what, err.max(axis=0), allow_p, allow_a)
        # ---- the searches on the union
        flat = lambda res: [np.asarray(x[key]) for x in res for key in sorted(x) if key != "hyp"] + [np.asarray(y[key]) for x in res for y in x.get("hyp", []) for key in sorted(y)]
        for name, call in (("alego_loop_search", lambda s: h.loop_search([s])), ("alego_loop_search_appearance", lambda s: h.loop_search_appearance([s])),
                           ("alego_map_align", lambda s: h.map_align([(0, s)]))):
            a, b = flat(call(D)), flat(call(RP))
            assert len(a) == len(b) > 0
            for x, y in zip(a, b):
                assert_bit_equal(x, y, f"lap: {name} on the union and on the replica")
    finally:
        h.close()


@pytest.mark.gpu
def test_replay_merge_agrees_with_the_binding(tmp_path):
    """examples/replay 150 --align 30 --merge: the align line, then the merge line, equal what the binding's calls give; --save-map holds the union"""
    n, start2 = 150, 30
    exe = os.path.join(ROOT, "examples", "replay")
    out = subprocess.run([exe, str(n), "--align", str(start2), "--merge", "--save-map", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith(("align:", "merge:"))]
    p = synth.default_params(16, 1800)
    h = binding.Handle(p, n_slots=2)
    try:
        h.map_enable(4096, 1 << 24)
        h.graph_enable(binding.ALIGN_MAX_QUERIES)
        h.loop_appearance_enable()
        for k in range(n):
            h.scan_process(_scan(p, k), stages=7, slot=0, stamp=0.1 * k)
            h.scan_process(_scan(p, start2 + k), stages=7, slot=1, stamp=0.1 * k)
        r = h.map_align([(1, 0)])[0]
        assert r["status"] == 2
        m = h.map_merge([(1, 0)], r["T"], seam_variance=SEAM, hyps=[r["hyp"]])[0]
        g = h.graph_optimize([0], apply=True)[0]
        want = [f"align: status {r['status']} queries {r['n_queries']} accepted {r['n_accepted']} support {r['support']} T" + "".join(f" {v:.9g}" for v in np.asarray(r["T"]).reshape(12)),
                f"merge: status {m['status']} frames {m['frames']} points {m['points']} loop_edges {m['loop_edges']} cross_edges {m['cross_edges']} optimise status {g['status']} "
                f"poses {g['n_poses']} loops {g['n_loops']} iterations {g['iterations']} cost {g['cost0']:.9g} -> {g['cost']:.9g}"]
        print("\n".join(got))
        assert got == want, (got, want)
        assert m["status"] == 2 and m["cross_edges"] >= 2 and g["status"] == 2 and g["applied"] == 1
        hdr = open(os.path.join(str(tmp_path), "keypose.pcd"), "rb").read(400).decode(errors="replace")
        assert f"POINTS {h.map_status(0)[0]}" in hdr and h.map_status(0)[0] == g["n_poses"], hdr
    finally:
        h.close()
