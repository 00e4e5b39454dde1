"""-m gpu: LaserMapping at pcl::VoxelGrid's "leaf size too small" rule (dx * dy * dz > INT_MAX: the cloud is returned unchanged).

The scenes (tests/util.py, PASS_SCENES) reach the rule in every VoxelGrid of LaserMapping: the local maps at the window level (map_update's
pass branch; the radix path's vox_big), the current scan's clouds and laser_surf_total_ (vox_small / vox_big), and a single key frame beyond
the rule (the key-frame sort, VoxJob mode 1).  Each scene asserts its own premise on the oracle; every mapping frame is compared with
_lm_compare (maps, k-NN rows, blocks, params_) and the map pose.
"""
import numpy as np
import pytest

from alego_amd import binding, synth
from oracle import oracle_py as O
from test_gpu_parity import POSE_TOL, _lm_compare
from test_global_map import ALL
from util import PASS_SCENES, assert_bit_equal, assert_pass_scene_premise, pass_correction, pass_scene, quat_angle

pytestmark = pytest.mark.gpu
LI_NREBUILD, LI_MAP_PASS = 24, 37   # (lm_ctx.h)


@pytest.mark.parametrize("outer", [1, 2])
@pytest.mark.parametrize("map_path", ["merge", "radix", "switching"])
@pytest.mark.parametrize("name", PASS_SCENES)
def test_lm_pass_through_scenes(name, map_path, outer):
    """Every scene on the merge path (pre-sorted key frames, incrementally kept voxel lists), on the concat + radix path (ALEGO_MAP_MERGE=0)
    and switching between them every two frames, with one and two outer iterations.  lm_info[LI_MAP_PASS] (bit m: map m passed through in
    map_update) must match the oracle wherever the merge path built the map.  (Before the fix, the key-frame sort reported a key frame beyond
    the rule as ALEGO_ERR_CAPACITY, and map_update merged the unsorted frame into its voxel lists while the window passed through.)"""
    scene = pass_scene(name)
    p = synth.default_params(16, 1800)
    for k, v in scene["mods"].items():
        setattr(p, k, v)
    p.lm_outer_iters = outer
    h, o = binding.Handle(p), O.Oracle(p)
    if map_path == "radix":
        h.set_option("ALEGO_MAP_MERGE", 0)
    for kp, c, s, ol in scene["keyframes"]:
        o.lm_add_keyframe(kp, c, s, ol)
        h.lm_add_keyframe(kp, c, s, ol)
    merge_built, nrebuild = False, 0
    for i, (c, s, ol, od) in enumerate(scene["frames"]):
        merge = map_path == "merge" or (map_path == "switching" and (i // 2) % 2 == 0)
        if map_path == "switching":
            h.set_option("ALEGO_MAP_MERGE", int(merge))
        tag = f"{name} {map_path} outer {outer} frame {i}"
        h.set_lm_params(o.get("lm_params"))
        o.lm_process(c, s, ol, od)
        flags, mp = h.lm_process(c, s, ol, dict(t=od[:3], q=od[3:]))
        assert_pass_scene_premise(name, scene, o, i)
        _lm_compare(h, o, i, tag)
        want = o.get("map_pose")
        assert np.abs(mp["t"] - want[:3]).max() < POSE_TOL and quat_angle(mp["q"], want[3:]) < POSE_TOL, tag
        gi = h.debug_get("lm_info")
        if gi[LI_NREBUILD] != nrebuild:   # the maps were built this frame, by the path that ran
            merge_built, nrebuild = merge, gi[LI_NREBUILD]
        if i in scene["expect"] and merge_built:
            want_bits = int(scene["expect"][i][0]) | (int(scene["expect"][i][1]) << 1)
            assert gi[LI_MAP_PASS] == want_bits, f"{tag}: lm_info[LI_MAP_PASS] = {gi[LI_MAP_PASS]} vs {want_bits}"
        if i == scene.get("correct_after"):
            nkf = h.lm_keyframe_count()
            poses, rc = pass_correction(o.get("lm_keyposes"))
            for k, q in enumerate(poses):
                o.lm_set_keypose(k, q)
                if k >= nkf - p.recent_keyframe_num:
                    h.lm_set_keypose(k, q)
            o.lm_reset_window(); h.lm_reset_window()
            o.lm_apply_correction(rc); h.lm_apply_correction(rc)
    assert h.lm_keyframe_count() == o.get("lm_info")[11]
    h.close()


def test_batch_replay_with_pass_through_slots_matches_single_slot_replicas():
    """The map_accum work list skips a slot whose map passed through (map_update's planner, LI_MAP_PASS): in a batch replay where every other
    slot plays the synthetic lap scaled by 4 (its scans and windows cross the rule at corner leaf 0.05, those of the plain lap do not), no slot
    reports an error, and the first two and the last slot of every stream group equal single-slot replicas bit for bit: global maps (every key
    pose of the run), the last local maps, lm_info and params_.  The premise (scaled: every map passes through, plain: none) is asserted on the
    oracle.  (A 10-key-frame window keeps every group's map_accum work list within its capacity.)"""
    from util import pcl_passes
    p = synth.default_params(16, 1800)
    p.min_keyframe_dist = 0.0
    p.lm_leaf_corner = 0.05
    p.recent_keyframe_num = 10
    bag_len, steps, n_slots, scale = 48, 40, 128, 4.0
    plain = [synth.scan(p, k) for k in range(bag_len)]
    scaled = [np.c_[s[:, :3] * scale, s[:, 3:]].astype(np.float32) for s in plain]
    for bag, scans in ((0, plain), (1, scaled)):
        o = O.Oracle(p)
        npass = 0
        for k in range(16):
            o.process_scan(scans[k])
            raw = o.get("lm_corner_map")
            if o.get("lm_info")[0] and len(raw):
                npass += int(pcl_passes(raw, p.lm_leaf_corner))
                assert (len(o.get("lm_corner_map_ds")) == len(raw)) >= pcl_passes(raw, p.lm_leaf_corner)
        assert npass == (7 if bag == 1 else 0), f"bag {bag}: {npass} of the first 16 scans pass through"   # (every mapping frame with a map)

    def replay(n, assign):
        h = binding.Handle(p, n_slots=n)
        h.replay_create(2, bag_len)
        for k in range(bag_len):
            h.replay_load(0, k, plain[k])
            h.replay_load(1, k, scaled[k])
        for s in range(n):
            h.replay_assign(s, *assign(s))
        h.map_enable(64, 1 << 18)
        return h

    of = lambda s: (s % 2, (s * 7) % bag_len)
    h = replay(n_slots, of)
    groups, per = h.stream_groups()
    assert groups >= 2
    h.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=False)
    h.synchronize()
    for s in range(n_slots):
        h.batch_get_pose(s)   # (raises on a capacity error of the slot)
    seen_pass = 0
    for g in range(groups):
        for s in (g * per, g * per + 1, min(n_slots, (g + 1) * per) - 1):
            r = replay(1, lambda _: of(s))
            r.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=True)
            r.batch_get_pose(0)
            assert h.map_status(s)[:3] == r.map_status(0)[:3] and r.map_status(0)[0] >= 5, (s, h.map_status(s), r.map_status(0))
            assert_bit_equal(h.map_assemble(ALL, slot=s), r.map_assemble(ALL), f"slot {s} global map")
            for name in ("lm_corner_map_ds", "lm_surf_map_ds", "lm_info"):
                assert_bit_equal(h.debug_get(name, slot=s), r.debug_get(name), f"slot {s} {name}")
            assert_bit_equal(h.debug_get("lm_state", slot=s)[0:6], r.debug_get("lm_state")[0:6], f"slot {s} params_")
            seen_pass += int(r.debug_get("lm_info")[LI_MAP_PASS] != 0)
            r.close()
    assert seen_pass > 0, "no compared slot ended with a map that passed through"
    h.close()
