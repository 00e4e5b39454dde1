"""-m gpu: LaserMapping's merge-path local map (map_update / map_accum, kernels_map.hip) at the edges of its own structure.

The scenes (tests/util.py, MERGE_SCENES) put known run sizes and known voxel-list positions in front of the kernels: run sizes at MU_FCAP and one
beyond (fast path / general path with a removal), lists of MU_E, MU_T * MU_E and MU_T * MU_E + 1 entries with voxels emptied and inserted on the
thread-interval boundaries, maps of 1, MAP_R - 1 .. 2 MAP_R + 1 voxels (work-item boundaries of map_accum), a voxel whose run exceeds a batch of
MA_BCAP points and batch cuts one before, on and one after a voxel change, zero-length runs and empty lists, and windows at the limits of the 21-bit
voxel key.  Each frame asserts its premise on the oracle's outputs and is compared with _lm_compare (maps bit for bit, k-NN rows, blocks, params_).
"""
import numpy as np
import pytest

from alego_amd import binding, synth
from oracle import oracle_py as O
from test_gpu_parity import POSE_TOL, _lm_compare
from util import MERGE_SCENES, assert_bit_equal, assert_merge_scene_premise, merge_scene, quat_angle

pytestmark = pytest.mark.gpu
LI_KRAW_C, LI_NREBUILD, LI_OVERFLOW, LI_NU_C, LI_MAP_PASS = 12, 24, 25, 28, 37   # (lm_ctx.h)


@pytest.mark.parametrize("map_path", ["merge", "switching"])
@pytest.mark.parametrize("name", MERGE_SCENES)
def test_lm_merge_scenes(name, map_path):
    """Every scene on the merge path and switching between it and the concat + radix path every two frames (the same sizes then also go through the
    rebuild of the voxel lists from nothing).  Per frame: the scene's premise on the oracle, _lm_compare, the map pose, and lm_info: list sizes equal
    to the filtered maps', raw counts, no pass-through, no overflow, one rebuild per changed window.

    A window with a voxel outside the 21-bit key range (far_*: want["raises"]) cannot be built by the merge path: the lm_process call that would
    build it raises ALEGO_ERR_CAPACITY with a message that names the voxel-key range, and the handle goes on to match the oracle on the following
    in-range windows.  (The radix path orders by box-relative voxel ids and builds such a window correctly; "switching" expects the error only on
    its merge frames.  Before the check, map_update clamped the cells beyond the range onto the last one and reported nothing: on the MI355X the
    surf maps of far_pos frames 4 - 8 came out with 512, 504, 504, 256 and 512 voxels against the oracle's 520, 512, 760, 512 and 768.)"""
    scene = merge_scene(name)
    p = synth.default_params(16, 1800)
    for k, v in scene["mods"].items():
        setattr(p, k, v)
    h, o = binding.Handle(p), O.Oracle(p)
    nrebuild, raised = 0, 0
    for i, (c, s, ol, od) in enumerate(scene["frames"]):
        merge = map_path == "merge" or (i // 2) % 2 == 0
        if map_path == "switching":
            h.set_option("ALEGO_MAP_MERGE", int(merge))
        tag = f"{name} {map_path} frame {i}"
        h.set_lm_params(o.get("lm_params"))
        o.lm_process(c, s, ol, od)
        facts = assert_merge_scene_premise(name, scene, o, i)
        if facts and facts.get("raises") and merge:
            with pytest.raises(binding.AlegoError, match=rf"\({binding.ERR_CAPACITY}\).*voxel-key range"):
                h.lm_process(c, s, ol, dict(t=od[:3], q=od[3:]))
            raised += 1
            gi = h.debug_get("lm_info")
            assert gi[LI_OVERFLOW] == 0 and gi[0] == o.get("lm_info")[11], f"{tag}: after the error: {gi[LI_OVERFLOW]}, {gi[0]} key frames"
            assert gi[LI_NREBUILD] == nrebuild + 1, f"{tag}: lm_info[LI_NREBUILD] = {gi[LI_NREBUILD]} after {nrebuild}"
            nrebuild = gi[LI_NREBUILD]
            # the refused map has no list and no points (lm_info[LI_MAP_PASS] bit 2 + m); a map of the same window that fits was built
            assert gi[LI_MAP_PASS] == sum(4 << m for m in range(2) if facts["refused"][m]), f"{tag}: lm_info[LI_MAP_PASS] = {gi[LI_MAP_PASS]}, refused {facts['refused']}"
            for m, ds_name in enumerate(("lm_corner_map_ds", "lm_surf_map_ds")):
                if facts["refused"][m]:
                    assert gi[LI_NU_C + m] == 0 and len(h.debug_get(ds_name)) == 0, f"{tag}: {ds_name} of a refused window: {gi[LI_NU_C + m]}, {len(h.debug_get(ds_name))}"
                else:
                    assert_bit_equal(h.debug_get(ds_name), o.get(ds_name), f"{tag} {ds_name} (the other map was refused)")
            continue
        flags, mp = h.lm_process(c, s, ol, dict(t=od[:3], q=od[3:]))
        _lm_compare(h, o, i, tag)
        want = o.get("map_pose")
        assert np.abs(mp["t"] - want[:3]).max() < POSE_TOL and quat_angle(mp["q"], want[3:]) < POSE_TOL, tag
        gi = h.debug_get("lm_info")
        raw = [len(o.get("lm_corner_map")), len(o.get("lm_surf_map"))]
        ds = [len(o.get("lm_corner_map_ds")), len(o.get("lm_surf_map_ds"))]
        assert gi[LI_OVERFLOW] == 0, f"{tag}: lm_info[LI_OVERFLOW] = {gi[LI_OVERFLOW]}"
        assert list(gi[LI_KRAW_C:LI_KRAW_C + 2]) == raw, f"{tag}: raw counts {gi[LI_KRAW_C:LI_KRAW_C + 2]} vs {raw}"
        if merge:
            assert list(gi[LI_NU_C:LI_NU_C + 2]) == ds, f"{tag}: voxel lists of {gi[LI_NU_C:LI_NU_C + 2]} entries vs filtered maps of {ds}"
            assert gi[LI_MAP_PASS] == 0, f"{tag}: lm_info[LI_MAP_PASS] = {gi[LI_MAP_PASS]}"
            assert gi[LI_NREBUILD] == nrebuild + (i > 0), f"{tag}: lm_info[LI_NREBUILD] = {gi[LI_NREBUILD]} after {nrebuild} (the window changes on every frame but the first)"
        nrebuild = gi[LI_NREBUILD]
    assert raised == sum(1 for i, w in scene["want"].items() if w.get("raises") and (map_path == "merge" or (i // 2) % 2 == 0)), f"{name}: {raised} errors"
    assert h.lm_keyframe_count() == o.get("lm_info")[11]
    h.close()
