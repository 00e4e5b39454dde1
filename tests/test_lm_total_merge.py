"""-m gpu: lm_total_merge (ALEGO_LM_TOTAL_MERGE, the default) against the sequence it stands in for (lm_total, the second VoxelGrid round, the /outlier
job of the first) and against oracle_py.

One-slot handles are fed constructed corner / surf / outlier clouds through lm_process, one with the option on and one with it off: lm_surf_total_ds,
lm_outlier_ds, their counts, lm_info's overflow word and the returned pose must be bit-equal, and the handle with the option on goes through
_lm_compare.  Every frame states the path it was built for ("fast": the merge; "list": refused, the round-2 job on the VoxelGrid work list); the premise
is checked on the oracle's clouds (laser_surf_ds_ in key order, outliers within LT_OCAP, the union inside the key range and the leaf-too-small rule),
and lm_info's counters LI_TM_FAST / LI_TM_LIST say which path the kernel took.  LT_OCAP is read from csrc/vox_merge.h.

ns + no beyond total_cap cannot be reached: total_cap = kf_cap_surf + kf_cap_outlier and round 1 cuts each cloud at its own capacity.  The capacity
that can be crossed is laser_outlier_ds_'s own (kf_cap_outlier), by the counted filter and by the general one: both must cut and raise alike.
"""
import os
import re

import numpy as np
import pytest

from alego_amd import binding, synth
from oracle import oracle_py as O
from test_gpu_parity import _lm_compare
from util import assert_bit_equal, pass_scene, pcl_passes

pytestmark = pytest.mark.gpu
F32 = np.float32
LI_NCUR_S, LI_NCUR_O, LI_NTOTAL, LI_NTOTAL_DS, LI_OVERFLOW, LI_TM_FAST, LI_TM_LIST = 20, 21, 22, 23, 25, 40, 41   # (lm_ctx.h)
VKEY_B = 1 << 20


def _ocap():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "a-lego-loam_amd", "csrc", "vox_merge.h")
    with open(path) as f:
        found = re.findall(r"^[ \t]*#define[ \t]+LT_OCAP[ \t]+(\d+)\b", f.read(), re.M)
    assert len(found) == 1, f"vox_merge.h: {len(found)} numeric #defines of LT_OCAP"
    return int(found[0])


LT_OCAP = _ocap()
ID7 = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)   # identity odometry: t, q (w first)


def _cloud(xyz, rng=None):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    w = rng.uniform(0, 16, len(xyz)) if rng is not None else np.arange(len(xyz)) % 16
    return np.c_[xyz, w].astype(F32)


def _cells(ix, iy, iz, leaf, rng, per=1, jitter=0.3):
    """`per` points in each cell (ix, iy, iz) of the leaf lattice, jittered around the centre"""
    c = np.stack(np.broadcast_arrays(ix, iy, iz), -1).reshape(-1, 3).astype(np.float64)
    c = np.repeat(c, per, axis=0)
    return (c + 0.5 + rng.uniform(-jitter, jitter, c.shape)) * leaf


def _keys(pts, leaf):
    inv = F32(1.0) / F32(leaf)
    c = np.floor(pts[:, :3].astype(F32) * inv).astype(np.int64)
    return c, ((c[:, 2] + VKEY_B) << 42) | ((c[:, 1] + VKEY_B) << 21) | (c[:, 0] + VKEY_B)


def _fast_expected(o, leaf_s):
    """vox_merge.h's vm_refuse restated on the oracle's clouds"""
    S, Oc = o.get("lm_surf_ds"), o.get("lm_outlier_ds")
    allp = np.r_[S, Oc]
    if len(allp) == 0:
        return True
    if len(Oc) > LT_OCAP or not np.isfinite(allp[:, :3]).all():
        return False
    cs, ks = _keys(S, leaf_s)
    if (np.diff(ks) < 0).any():
        return False
    ca, _ = _keys(allp, leaf_s)
    if ca.min() < -VKEY_B or ca.max() > VKEY_B - 1 or pcl_passes(allp[:, :3], leaf_s):
        return False
    return float(np.prod((ca.max(0) - ca.min(0) + 1).astype(np.float64))) <= 0xFFFFFFFF


E1, E2 = F32(5.5999994), F32(-1.6000001)   # three equal points there average into the next 0.8 m cell


def _frames(leaf_o):
    """(name, corner, surf, outlier, path) at lm_leaf_surf 0.8"""
    rng = np.random.default_rng(19)
    LS = 0.8
    corner = _cloud(rng.uniform(-10, 10, (30, 3)), rng)
    base_s = _cloud(_cells(np.arange(12)[:, None], np.arange(10)[None, :], 0, LS, rng, per=3), rng)   # 120 voxels of 3 points
    out41 = _cloud(np.c_[rng.uniform(-3, 13, 41), rng.uniform(-3, 11, 41), rng.uniform(-1.5, 2.5, 41)], rng)
    fr = [("plain", corner, base_s, out41, "fast")]
    for e in (E1, E2, -E1, -E2):   # the escape triple on x, an outlier in the cell it left and one in the cell it reached, neighbours around
        tri = np.array([[e, 0.1, 4.1]] * 3, F32)
        s = np.r_[base_s, _cloud(tri, rng)]
        o = _cloud([[e, 0.2, 4.2], [float(e) + 0.05, 0.3, 4.3], [1.0, 1.0, 1.0]], rng)
        fr.append((f"escape_x_{float(e):.3f}", corner, s, o, "fast"))
    tri = np.array([[E1, 0.1, 4.1]] * 3 + [[5.7, 0.1, 4.1]], F32)   # ... into an occupied neighbour: two centroids share a cell and merge
    fr.append(("escape_occupied", corner, np.r_[base_s, _cloud(tri, rng)], _cloud([[5.9, 0.3, 4.3], [5.0, 0.3, 4.3]], rng), "fast"))
    tri = np.array([[3.0, E1, 4.1]] * 3 + [[5.0, 5.0, 4.1]], F32)   # ... backwards: the y cell grows past a later voxel of the old y cell
    fr.append(("escape_breaks_order", corner, np.r_[base_s, _cloud(tri, rng)], out41, "list"))
    zs = _cloud([[-0.0, -0.0, -0.0], [1.0, -0.0, 0.0], [-0.0, 3.0, -0.0]])   # -0.f alone in its voxel comes out +0.f
    zs[:, 3] = [-0.0, 1.0, -0.0]
    fr.append(("minus_zero", corner, zs, _cloud([[-0.0, 5.0, -0.0], [-0.0, 5.1, 0.0]]), "fast"))
    fr.append(("o_before_after_inside", corner, base_s, _cloud([[-5, 0, -3], [-4, 0, -3], [0, 0, 9], [0, 1, 9], [4.3, 1.3, 0.3], [100, 0.3, 0.3]], rng), "fast"))
    fr.append(("o_shares_voxels", corner, base_s, _cloud([[4.1, 0.1, 0.1], [4.2, 0.2, 0.2], [4.3, 0.7, 0.1], [4.1, 20.1, 0.1], [4.2, 20.2, 0.2], [4.25, 20.25, 0.2]], rng), "fast"))
    empty = np.zeros((0, 4), F32)
    fr += [("empty_o", corner, base_s, empty, "fast"), ("empty_s", corner, empty, out41, "fast"), ("both_empty", corner, empty, empty, "fast")]
    # raw outliers around LT_OCAP, one per cell of a 1 m lattice at z = 2 (distinct cells at both outlier leaves); with two in one cell: no = raw - 1
    cell = lambda n: np.c_[(np.arange(n) % 32) + 0.5, (np.arange(n) // 32) + 0.5, np.full(n, 2.5)]
    for n, dup, path in ((LT_OCAP - 1, 0, "fast"), (LT_OCAP, 0, "fast"), (LT_OCAP + 1, 0, "list"), (LT_OCAP + 1, 1, "fast"), (LT_OCAP + 2, 1, "list"), (LT_OCAP + 90, 91, "fast")):
        xyz = cell(n - dup)
        xyz = np.r_[xyz, xyz[:dup] + 0.01]
        fr.append((f"outliers_{n}_filtered_{n - dup}", corner, base_s, _cloud(xyz, rng), path))
    fr.append(("cell_beyond_key_range", corner, base_s, _cloud([[1.0e6, 0, 0], [1, 1, 1]], rng), "list"))
    fr.append(("leaf_too_small_union", corner, base_s, _cloud([[2500, 2500, 2500], [1, 1, 1]], rng), "list"))
    fr.append(("plain_again", corner, base_s + F32(0.01), out41, "fast"))
    return fr


def _pair(p):
    h1, h0 = binding.Handle(p), binding.Handle(p)
    h0.set_option("ALEGO_LM_TOTAL_MERGE", 0)
    return h1, h0


def _same(h1, h0, r1, r0, tag, slot=0):
    for name in ("lm_surf_total_ds", "lm_outlier_ds", "lm_surf_ds", "lm_corner_ds"):
        assert_bit_equal(h1.debug_get(name, slot=slot), h0.debug_get(name, slot=slot), f"{tag} {name}, ALEGO_LM_TOTAL_MERGE 1 vs 0")
    g1, g0 = h1.debug_get("lm_info", slot=slot), h0.debug_get("lm_info", slot=slot)
    assert list(g1[:LI_TM_FAST]) == list(g0[:LI_TM_FAST]), f"{tag}: lm_info {list(g1[:LI_TM_FAST])} vs {list(g0[:LI_TM_FAST])}"
    if r1 is not None:
        assert r1[0] == r0[0], f"{tag}: flags {r1[0]} vs {r0[0]}"
        for k in ("t", "q"):
            assert_bit_equal(np.asarray(r1[1][k]), np.asarray(r0[1][k]), f"{tag} map pose {k}")
    return g1, g0


@pytest.mark.parametrize("leaf_o", [1.0, 0.8])
def test_constructed_clouds_equal_the_second_round_and_the_oracle(leaf_o):
    """Every built frame with lm_leaf_outlier 1.0 and 0.8 (= lm_leaf_surf): option on == option off bit for bit, == the oracle, and the counters name
    the path the frame was built for.  The registration guard is closed (lm_min_corner above any cloud): the frames are about the clouds."""
    p = synth.default_params(16, 1800)
    p.lm_leaf_surf, p.lm_leaf_outlier, p.lm_min_corner, p.lm_every = 0.8, leaf_o, 1 << 20, 1
    h1, h0 = _pair(p)
    o = O.Oracle(p)
    fast = lst = 0
    for i, (name, c, s, ol, path) in enumerate(_frames(leaf_o)):
        tag = f"leaf_o {leaf_o} frame {i} {name}"
        o.lm_process(c, s, ol, ID7)
        assert _fast_expected(o, 0.8) == (path == "fast"), f"{tag}: premise: the frame was built for the {path} path"
        if name.startswith("escape_x") and name.split("_")[-1] in ("5.600", "-1.600"):
            S = o.get("lm_surf_ds")
            assert (S[:, 0] == F32(float(name.split("_")[-1]))).any(), f"{tag}: premise: no centroid at the cell boundary"
        if name.startswith("outliers_"):
            assert (len(ol), len(o.get("lm_outlier_ds"))) == tuple(int(v) for v in name.split("_")[1::2]), f"{tag}: premise: {len(ol)} raw, {len(o.get('lm_outlier_ds'))} filtered"
        r1 = h1.lm_process(c, s, ol, dict(t=ID7[:3], q=ID7[3:]))
        r0 = h0.lm_process(c, s, ol, dict(t=ID7[:3], q=ID7[3:]))
        g1, g0 = _same(h1, h0, r1, r0, tag)
        _lm_compare(h1, o, i, tag)
        assert g1[LI_OVERFLOW] == 0 and g1[LI_NCUR_O] == len(o.get("lm_outlier_ds")) and g1[LI_NTOTAL_DS] == len(o.get("lm_surf_total_ds")), tag
        assert g1[LI_NTOTAL] == g1[LI_NCUR_S] + g1[LI_NCUR_O], tag
        fast, lst = fast + (path == "fast"), lst + (path == "list")
        assert (g1[LI_TM_FAST], g1[LI_TM_LIST]) == (fast, lst), f"{tag}: built for the {path} path; counters {g1[LI_TM_FAST]}, {g1[LI_TM_LIST]} after {fast}, {lst}"
        assert (g0[LI_TM_FAST], g0[LI_TM_LIST]) == (0, 0), f"{tag}: ALEGO_LM_TOTAL_MERGE 0 ran lm_total_merge"
        if name == "minus_zero":
            assert not np.signbit(h1.debug_get("lm_surf_total_ds")).any(), f"{tag}: a -0.f survived the filter"
    assert fast > 0 and lst > 0
    h1.close(); h0.close()


@pytest.mark.parametrize("first,period", [(1, 1), (0, 1), (1, 2), (0, 2), (0, 3)])
def test_switching_the_option_between_frames(first, period):
    """ALEGO_LM_TOTAL_MERGE switched by set_option while one handle runs the built frames (refused ones among them): `period` frames with the option at
    `first`, `period` with the other value, and so on, so lm_total_merge comes back after odd and after even numbers of its own launches and of
    the second VoxelGrid round's, whose vox_plan writes list sizes of its own.  lm_total_merge's list counters must not see them: every frame equals
    the oracle, and the counters count exactly the frames that ran with the option on, each on the path it was built for.  (With shared counters a
    merge frame behind a round-2 frame ran the stale list over laser_surf_total_ds_, and a refused slot appended behind it.)"""
    p = synth.default_params(16, 1800)
    p.lm_leaf_surf, p.lm_leaf_outlier, p.lm_min_corner, p.lm_every = 0.8, 1.0, 1 << 20, 1
    h, o = binding.Handle(p), O.Oracle(p)
    fast = lst = 0
    seen = set()
    prev_on = None
    for i, (name, c, s, ol, path) in enumerate(_frames(1.0)):
        on = first ^ ((i // period) % 2)
        h.set_option("ALEGO_LM_TOTAL_MERGE", on)
        tag = f"first {first} period {period} frame {i} {name} option {on}"
        o.lm_process(c, s, ol, ID7)
        h.lm_process(c, s, ol, dict(t=ID7[:3], q=ID7[3:]))
        _lm_compare(h, o, i, tag)
        gi = h.debug_get("lm_info")
        assert gi[LI_OVERFLOW] == 0 and gi[LI_NTOTAL_DS] == len(o.get("lm_surf_total_ds")) and gi[LI_NCUR_O] == len(o.get("lm_outlier_ds")), tag
        fast, lst = fast + (on and path == "fast"), lst + (on and path == "list")
        assert (gi[LI_TM_FAST], gi[LI_TM_LIST]) == (fast, lst), f"{tag}: counters {gi[LI_TM_FAST]}, {gi[LI_TM_LIST]} after {fast}, {lst}"
        if prev_on is not None and prev_on != on:
            seen.add((on, path))
        prev_on = on
    assert {(1, "fast"), (1, "list"), (0, "fast"), (0, "list")} <= seen, f"switches seen: {sorted(seen)}"   # both paths right behind a switch, either way
    h.close()


def test_pass_through_first_round_goes_to_the_list():
    """PASS_SCENES' scan_small: every cloud of the scan crosses the leaf-too-small rule in round 1 (laser_surf_ds_ comes back unsorted, more than
    LT_OCAP outliers), so every frame is refused; the registration runs.  Both handles equal each other and the oracle."""
    scene = pass_scene("scan_small")
    p = synth.default_params(16, 1800)
    for k, v in scene["mods"].items():
        setattr(p, k, v)
    h1, h0 = _pair(p)
    o = O.Oracle(p)
    for kp, c, s, ol in scene["keyframes"]:
        o.lm_add_keyframe(kp, c, s, ol); h1.lm_add_keyframe(kp, c, s, ol); h0.lm_add_keyframe(kp, c, s, ol)
    for i, (c, s, ol, od) in enumerate(scene["frames"]):
        tag = f"scan_small frame {i}"
        for h in (h1, h0):
            h.set_lm_params(o.get("lm_params"))
        o.lm_process(c, s, ol, od)
        assert len(o.get("lm_surf_ds")) == len(s) and not _fast_expected(o, p.lm_leaf_surf), f"{tag}: premise: round 1 passes through"
        r1 = h1.lm_process(c, s, ol, dict(t=od[:3], q=od[3:]))
        r0 = h0.lm_process(c, s, ol, dict(t=od[:3], q=od[3:]))
        g1, _ = _same(h1, h0, r1, r0, tag)
        _lm_compare(h1, o, i, tag)
        assert (g1[LI_TM_FAST], g1[LI_TM_LIST]) == (0, i + 1), f"{tag}: counters {g1[LI_TM_FAST]}, {g1[LI_TM_LIST]}"
    h1.close(); h0.close()


def test_outlier_capacity_cuts_and_raises_alike():
    """kf_cap_outlier 300: 305 and LT_OCAP + 5 outliers in cells of their own overflow laser_outlier_ds_ in the counted filter and in the general one;
    both handles raise ALEGO_ERR_CAPACITY and leave the same 300 points, counts and merged cloud."""
    p = synth.default_params(16, 1800)
    p.kf_cap_outlier, p.lm_min_corner, p.lm_every = 300, 1 << 20, 1
    h1, h0 = _pair(p)
    rng = np.random.default_rng(5)
    corner = _cloud(rng.uniform(-10, 10, (30, 3)), rng)
    surf = _cloud(_cells(np.arange(12)[:, None], np.arange(10)[None, :], 0, 0.8, rng, per=3), rng)
    for n in (305, LT_OCAP + 5):
        ol = _cloud(np.c_[(np.arange(n) % 32) + 0.5, (np.arange(n) // 32) + 0.5, np.full(n, 2.5)], rng)
        for h in (h1, h0):
            with pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_CAPACITY}\)"):
                h.lm_process(corner, surf, ol, dict(t=ID7[:3], q=ID7[3:]))
        g1, _ = _same(h1, h0, None, None, f"{n} outliers")
        assert g1[LI_NCUR_O] == 300 and g1[LI_NTOTAL] == g1[LI_NCUR_S] + 300, f"{n} outliers: {g1[LI_NCUR_O]} kept, {g1[LI_NTOTAL]} merged"
    h1.close(); h0.close()


def test_three_slots_refused_between_accepted():
    """A 3-slot batch replay at lm_leaf_surf 0.1: slots 0 and 2 play the synthetic lap, slot 1 the lap scaled by 8, whose surf cloud crosses the
    leaf-too-small rule in round 1 (premise on the oracle) and is refused on every mapping frame, between two slots that merge.  lm_every 2: every
    other scan no slot maps: the host skips the whole mapping sequence of such a view, lm_total_merge included (a launch whose slots all have their
    run flag clear does not occur; a slot that does not run inside a launch that does takes the kernel's LI_RUN == 0 exit, as slots of a view do in other tests).  Option on == option off for every slot; the counters name each slot's path."""
    p = synth.default_params(16, 1800)
    p.lm_leaf_surf, p.kf_cap_surf = 0.1, 16 * 1800   # (the scaled lap's unfiltered surf cloud is larger than the default capacity of laser_surf_ds_)
    bag_len, steps, scale = 12, 12, 8.0
    plain = [synth.scan(p, k) for k in range(bag_len)]
    scaled = [np.c_[s[:, :3] * scale, s[:, 3:]].astype(F32) for s in plain]
    for scans, passes in ((plain, False), (scaled, True)):
        o = O.Oracle(p)
        seen = 0
        for k in range(4):
            o.process_scan(scans[k])
            if o.get("lm_info")[0]:
                assert pcl_passes(o.get("lm_surf_ds")[:, :3], p.lm_leaf_surf) == passes and _fast_expected(o, p.lm_leaf_surf) == (not passes), f"premise: scan {k}, scale {passes}"
                seen += 1
        assert seen >= 2

    def replay(merge):
        h = binding.Handle(p, n_slots=3)
        h.set_option("ALEGO_LM_TOTAL_MERGE", merge)
        h.replay_create(2, bag_len)
        for k in range(bag_len):
            h.replay_load(0, k, plain[k]); h.replay_load(1, k, scaled[k])
        for s in range(3):
            h.replay_assign(s, s % 2, s)
        h.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=True)
        return h

    h1, h0 = replay(1), replay(0)
    for s in range(3):
        r1, r0 = h1.batch_get_pose(s), h0.batch_get_pose(s)
        g1, g0 = _same(h1, h0, (r1[0], r1[2]), (r0[0], r0[2]), f"slot {s}", slot=s)
        assert_bit_equal(h1.debug_get("lm_state", slot=s)[0:6], h0.debug_get("lm_state", slot=s)[0:6], f"slot {s} params_")
        frames = steps // 2
        want = (0, frames) if s == 1 else (frames, 0)
        assert (g1[LI_TM_FAST], g1[LI_TM_LIST]) == want, f"slot {s}: counters {g1[LI_TM_FAST]}, {g1[LI_TM_LIST]}, wanted {want}"
        assert (g0[LI_TM_FAST], g0[LI_TM_LIST]) == (0, 0)
    h1.close(); h0.close()
