"""LaserOdometry's correspondence search (lo_assoc, laserOdometry.cpp:337-481) query by query on constructed segmented clouds.

Each scene is two segmented clouds fed to LaserOdometry directly: scan 0 supplies the targets (less_flat / less_sharp), scan 1 the queries
(flat / sharp), with both sides teacher-forced to the same params_ and a zero solver budget.  The oracle's accepted rows must equal a plain numpy
restatement of the search (lo_assoc_brute); on the GPU every row lo_assoc writes — rejected rows with their partial walk results included —
must equal it too, on the default path, without the target grid, with the boxes read from HBM, and with the other feature-extraction box writer.
"""
import numpy as np
import pytest

from util import (LO_SCENES, LO_SCENES_BIG, assert_bit_equal, assert_lo_scene_premise, build_lo_scene, lo_assoc_brute, run_lo_scene_oracle)

GEOMS = [(16, 1800), (64, 2048)]
CASES = [(s, g) for g in GEOMS for s in LO_SCENES] + [(s, (64, 2048)) for s in LO_SCENES_BIG]


def _oracle_scene(name, geom):
    sc = build_lo_scene(name, geom)
    o = run_lo_scene_oracle(sc)
    rows = lo_assoc_brute(sc["less_flat"], sc["less_sharp"], o.get("flat"), o.get("sharp"), sc["params6"], sc["P"])
    return sc, o, rows


def _accepted_equal(o, rows, tag):
    surf, corner = rows
    assert_bit_equal(o.get("lo_surf_corr").reshape(-1, 4), surf[surf[:, 1] >= 0], f"{tag}: oracle surf rows vs the restatement")
    assert_bit_equal(o.get("lo_corner_corr").reshape(-1, 3), corner[corner[:, 1] >= 0][:, :3], f"{tag}: oracle corner rows vs the restatement")


@pytest.mark.parametrize("name,geom", CASES, ids=[f"{s}-{g[0]}x{g[1]}" for s, g in CASES])
def test_lo_scene_oracle_matches_brute(name, geom):
    sc, o, rows = _oracle_scene(name, geom)
    _accepted_equal(o, rows, name)
    assert_lo_scene_premise(name, sc, o, rows)
    o.close()


GPU_VARIANTS = [None, "ALEGO_LO_GRID", "ALEGO_LO_BOX_LDS", "ALEGO_FE_FUSED"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", GPU_VARIANTS, ids=["default", "nogrid", "hbm_boxes", "unfused_fe"])
@pytest.mark.parametrize("name,geom", CASES, ids=[f"{s}-{g[0]}x{g[1]}" for s, g in CASES])
def test_lo_scene_device(name, geom, variant, monkeypatch):
    """every device row of both searches equals lo_assoc_brute bit for bit (rejected rows and their partial idx2 / idx3 included)"""
    from alego_amd import binding
    from test_gpu_parity import _fe_compare
    if variant:
        monkeypatch.setenv(variant, "0")
    sc, o, rows = _oracle_scene(name, geom)
    from oracle import oracle_py as O
    ref = O.Oracle(sc["P"])   # a second oracle, stepped alongside the device for _fe_compare's per-scan outputs
    h = binding.Handle(sc["P"])
    for k, seg in enumerate((sc["seg0"], sc["seg1"])):
        if k:
            h.set_lo_params(sc["params6"])
            ref.set_lo_params(sc["params6"])
        ref.set_seg(seg)
        ref.lo()
        flags, feat, odom = h.lo_process(seg)
        _fe_compare(h, ref, feat, f"{name} scan {k}")
    surf, corner = rows
    assert_bit_equal(h.debug_get("lo_surf_corr").reshape(-1, 4), surf, f"{name} {variant}: surf rows")
    assert_bit_equal(h.debug_get("lo_corner_corr").reshape(-1, 4), corner, f"{name} {variant}: corner rows")
    assert_bit_equal(h.debug_get("lo_state")[18:24], sc["params6"], f"{name}: params after the surf solve")
    _accepted_equal(ref, rows, name)
    h.close(); ref.close(); o.close()
