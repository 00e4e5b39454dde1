"""The global map: key-frame archive (alego_map_*), map assembly, the device-wide VoxelGrid (alego_voxel_grid), the local-map
export and the PCD writer.  Reference results are composed from what the oracle already exports: its key frames
(Oracle.lm_keyframe, every frame, not only the resident window), its key poses, transform_cloud and voxel_grid(sort_mode = 0)."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal, tall_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER
GV_SMALL_MAX = 32768   # csrc/gmap.h GV_SMALL_MAX_DEFAULT: clouds up to this size take the one-workgroup kernels


# ---- CPU ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["alego_map_enable", "alego_map_status", "alego_map_set_keyposes", "alego_map_get_keyframe", "alego_map_assemble",
               "alego_map_keyposes", "alego_lm_get_local_map", "alego_voxel_grid", "alego_write_pcd"]


def test_header_and_library_have_the_map_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    L = binding.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in binding.EXPORTS, s


def read_pcd(path):
    raw = open(path, "rb").read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode()
        pos = end + 1
        if line.startswith("#"):
            continue
        k, _, v = line.partition(" ")
        head[k] = v
        if k == "DATA":
            break
    return head, raw[pos:]


@pytest.mark.parametrize("kind", ["empty", "one", "special", "many"])
def test_write_pcd_round_trip(tmp_path, kind):
    rng = np.random.default_rng(3)
    pts = {"empty": np.zeros((0, 4), np.float32),
           "one": np.array([[1.5, -2.25, 3.0, 7.0]], np.float32),
           "special": np.array([[np.nan, -0.0, 0.0, -1.0], [np.inf, -np.inf, 1e-45, np.nan], [-0.0, -0.0, -0.0, -0.0]], np.float32),
           "many": rng.normal(0, 100, (10007, 4)).astype(np.float32)}[kind]
    path = str(tmp_path / "c.pcd")
    binding.write_pcd(path, pts)
    head, data = read_pcd(path)
    n = pts.shape[0]
    assert head["VERSION"] == "0.7" and head["FIELDS"] == "x y z intensity" and head["SIZE"] == "4 4 4 4" and head["TYPE"] == "F F F F"
    assert head["COUNT"] == "1 1 1 1" and head["WIDTH"] == str(n) and head["HEIGHT"] == "1" and head["POINTS"] == str(n)
    assert head["VIEWPOINT"] == "0 0 0 1 0 0 0" and head["DATA"] == "binary"
    assert len(data) == n * 16
    assert_bit_equal(np.frombuffer(data, np.float32).reshape(-1, 4), pts, f"PCD data ({kind})")


def test_write_pcd_refuses_bad_arguments(tmp_path):
    L = binding.lib()
    assert L.alego_write_pcd(str(tmp_path / "x.pcd").encode(), None, 3) == binding.ERR_ARG
    assert L.alego_write_pcd(str(tmp_path / "no_such_dir" / "x.pcd").encode(), None, 0) == binding.ERR_ARG


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _O():
    from oracle import oracle_py
    return oracle_py


def oracle_map(o, nf, kinds, leaf=0.0, poses=None):
    """saveMapCB / visualizeGlobalMapThread composed from the oracle's key frames at `poses` (default: its own key poses)"""
    O = _O()
    poses = o.get("lm_keyposes").reshape(-1, 6) if poses is None else poses
    parts = [np.zeros((0, 4), np.float32)]
    for i in range(nf):
        c, s, ol = o.lm_keyframe(i)
        for bit, cl in ((binding.MAP_SURF, s), (binding.MAP_CORNER, c), (binding.MAP_OUTLIER, ol)):
            if kinds & bit and cl.shape[0]:
                t = O.transform_cloud(poses[i], cl)
                if kinds & binding.MAP_FRAME_ID:
                    t[:, 3] = np.float32(i)
                parts.append(t)
    cat = np.concatenate(parts)
    return O.voxel_grid(cat, leaf, 0) if leaf > 0 else cat


def check_maps(h, o, nf, tag, leaves=(0.2, 0.4, 1.0), poses=None, slot=0):
    for kinds in (binding.MAP_CORNER | binding.MAP_FRAME_ID, binding.MAP_SURF | binding.MAP_FRAME_ID, binding.MAP_OUTLIER | binding.MAP_FRAME_ID, ALL):
        assert_bit_equal(h.map_assemble(kinds, slot=slot), oracle_map(o, nf, kinds, poses=poses), f"{tag}: map kinds {kinds}")
    for leaf in leaves:
        assert_bit_equal(h.map_assemble(ALL, leaf, slot=slot), oracle_map(o, nf, ALL, leaf, poses=poses), f"{tag}: global map leaf {leaf}")
    kp = (o.get("lm_keyposes").reshape(-1, 6) if poses is None else poses)[:nf]
    want = np.concatenate([kp[:, :3], np.arange(nf, dtype=np.float32)[:, None]], axis=1).astype(np.float32)
    assert_bit_equal(h.map_keyposes(slot), want, f"{tag}: keypose.pcd")


SCANS = 70
CAP_POINTS = 60000   # ~22 of the 35 key frames of the run below (2.6-2.7 k points each)


@pytest.fixture(scope="module")
def archived_run():
    """A teacher-forced run (as test_keyframe_pass_through_and_pose_correction) with a window of 6 key frames and a key frame on every
    mapping frame; two handles see the same scans: one archives everything, one has a point capacity that fills mid-run."""
    O = _O()
    p = synth.default_params(16, 1800)
    p.recent_keyframe_num = 6
    p.min_keyframe_dist = 0.0
    h, hc, o = binding.Handle(p), binding.Handle(p), O.Oracle(p)
    h.map_enable(256, 1 << 20)
    hc.map_enable(256, CAP_POINTS)
    for k in range(SCANS):
        pts = synth.scan(p, k)
        for x in (h, hc):
            x.set_lo_params(o.get("lo_params"))
            x.set_lm_params(o.get("lm_params"))
        o.process_scan(pts)
        h.scan_process(pts, stages=7)
        hc.scan_process(pts, stages=7)
    yield p, h, hc, o
    h.close()
    hc.close()


@pytest.mark.gpu
def test_archive_keeps_every_key_frame(archived_run):
    p, h, _, o = archived_run
    nkf = h.lm_keyframe_count()
    assert nkf >= 30 and nkf == o.get("lm_keyposes").size // 6, nkf
    st = h.map_status()
    assert st[0] == nkf and st[1] == 0 and st[3] == 1 << 20
    poses = o.get("lm_keyposes").reshape(-1, 6)
    total = 0
    for i in range(nkf):
        kf = h.map_get_keyframe(i)
        oc, os_, oo = o.lm_keyframe(i)
        assert kf["id"] == i
        assert_bit_equal(kf["corner"], oc, f"archived frame {i} corner")
        assert_bit_equal(kf["surf"], os_, f"archived frame {i} surf")
        assert_bit_equal(kf["outlier"], oo, f"archived frame {i} outlier")
        assert_bit_equal(kf["pose"], poses[i], f"archived frame {i} pose")
        total += oc.shape[0] + os_.shape[0] + oo.shape[0]
    assert st[2] == total
    with pytest.raises(binding.AlegoError):
        h.lm_get_keyframe(0)   # the resident ring's contract is unchanged: frame 0 is long gone from it
    check_maps(h, o, nkf, "archive")
    c, s = h.lm_local_map()
    assert_bit_equal(c, o.get("lm_corner_map_ds"), "local corner map")
    assert_bit_equal(s, o.get("lm_surf_map_ds"), "local surf map")


@pytest.mark.gpu
def test_archive_capacity_keeps_a_prefix(archived_run):
    p, h, hc, o = archived_run
    nkf = hc.lm_keyframe_count()
    stored, dropped, npts, cap = hc.map_status()
    assert cap == CAP_POINTS and 0 < stored < nkf and stored + dropped == nkf, (stored, dropped, nkf)
    sizes = [sum(c.shape[0] for c in o.lm_keyframe(i)) for i in range(nkf)]
    assert npts == sum(sizes[:stored]) and npts + sizes[stored] > CAP_POINTS
    check_maps(hc, o, stored, "capacity", leaves=(0.4,))
    n = hc.map_assemble(ALL).shape[0]
    L = binding.lib()
    out = np.zeros((n, 4), np.float32)
    assert L.alego_map_assemble(hc._h, 0, ALL, 0.0, out.ctypes.data, n - 1) == binding.ERR_CAPACITY
    assert not out.any()
    assert L.alego_map_assemble(hc._h, 0, ALL, 0.0, None, 0) == n


@pytest.mark.gpu
def test_archive_pose_correction_and_inserted_frames(archived_run):
    """correctPoses over the whole graph: every archived pose rewritten (alego_map_set_keyposes), the resident ones also through
    alego_lm_set_keypose; then frames inserted by alego_lm_add_keyframe must appear in the map."""
    p, h, _, o = archived_run
    nkf = h.lm_keyframe_count()
    poses = o.get("lm_keyposes").reshape(-1, 6).copy()
    c, s = np.cos(0.03), np.sin(0.03)
    rc = np.array([[c, -s, 0, 0.4], [s, c, 0, -0.25], [0, 0, 1, 0.05]])
    new = poses.astype(np.float64)
    new[:, :3] = new[:, :3] @ rc[:, :3].T + rc[:, 3]
    new[:, 5] += 0.03
    new = new.astype(np.float32)
    h.map_set_keyposes(0, new)
    for i in range(nkf):
        o.lm_set_keypose(i, new[i])
        if i >= nkf - p.recent_keyframe_num:
            h.lm_set_keypose(i, new[i])
    assert_bit_equal(o.get("lm_keyposes").reshape(-1, 6), new, "oracle poses rewritten")
    check_maps(h, o, nkf, "corrected", leaves=(0.4,))
    with pytest.raises(binding.AlegoError):
        h.map_set_keyposes(nkf - 1, new[:2])   # beyond the archived frames
    # insert two frames (copies of old ones, at new poses), as a host pose graph restoring a session would
    h.lm_reset_window(); o.lm_reset_window()
    for j, src in enumerate((3, 11)):
        cl = o.lm_keyframe(src)
        pose = new[src] + np.float32(0.5 * (j + 1))
        h.lm_add_keyframe(pose, *cl)
        o.lm_add_keyframe(pose, *cl)
    assert h.lm_keyframe_count() == nkf + 2 and h.map_status()[0] == nkf + 2
    check_maps(h, o, nkf + 2, "inserted", leaves=(0.4,))


@pytest.mark.gpu
def test_batch_replay_global_maps_match_single_slot_replicas():
    p = synth.default_params(16, 1800)
    p.min_keyframe_dist = 0.0
    bag_len, steps, n_slots = 48, 40, 128
    scans = [synth.scan(p, k) for k in range(bag_len)]

    def replay(n, slots_of):
        h = binding.Handle(p, n_slots=n)
        h.replay_create(1, bag_len)
        for k, pts in enumerate(scans):
            h.replay_load(0, k, pts)
        for s in range(n):
            h.replay_assign(s, 0, slots_of(s))
        h.map_enable(64, 1 << 18)
        return h

    start = lambda s: (s * 7) % bag_len
    h = replay(n_slots, start)
    groups, per = h.stream_groups()
    assert groups >= 2
    h.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=False)   # no host call between the steps
    h.synchronize()
    for g in range(groups):
        for s in (g * per, min(n_slots, (g + 1) * per) - 1):
            r = replay(1, lambda _: start(s))
            r.batch_run(0, steps, stages=7 | binding.REPLAY_BAG, sync=True)
            assert h.map_status(s)[:3] == r.map_status(0)[:3] and r.map_status(0)[0] >= 5, (s, h.map_status(s), r.map_status(0))
            assert_bit_equal(h.map_assemble(ALL, slot=s), r.map_assemble(ALL), f"slot {s} global map")
            assert_bit_equal(h.map_assemble(ALL, 0.4, slot=s), r.map_assemble(ALL, 0.4), f"slot {s} global map, leaf 0.4")
            r.close()
    h.close()


VG_CASES = ["uniform_1M", "clustered_1M", "uniform_4M", "clustered_4M", "lattice_negative", "one_voxel_1e5",
            f"threshold_{GV_SMALL_MAX - 1}", f"threshold_{GV_SMALL_MAX}", f"threshold_{GV_SMALL_MAX + 1}", "n1",
            f"tall_{GV_SMALL_MAX // 2}", f"tall_{GV_SMALL_MAX * 2}"]   # more than 2^32 grid cells


def _vg_case(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))

    def cloud(xyz):
        return np.concatenate([xyz, rng.uniform(0, 100, (xyz.shape[0], 1))], axis=1).astype(np.float32)

    centers = rng.uniform(-80, 80, (200, 3))
    if name == "uniform_1M":
        return cloud(rng.uniform(-60, 40, (1 << 20, 3))), 0.4
    if name == "clustered_1M":
        return cloud(centers[rng.integers(0, 200, 1 << 20)] + rng.normal(0, 1.5, (1 << 20, 3))), 0.4
    if name == "uniform_4M":
        return cloud(rng.uniform(-100, 100, (1 << 22, 3))), 0.4
    if name == "clustered_4M":
        return cloud(centers[rng.integers(0, 200, 1 << 22)] + rng.normal(0, 2.0, (1 << 22, 3))), 0.4
    if name == "lattice_negative":   # negative coordinates on exact multiples of the leaf
        return cloud(rng.integers(-300, 50, (300000, 3)).astype(np.float32) * np.float32(0.25)), 0.25
    if name == "one_voxel_1e5":      # 10^5 points in one voxel, shuffled among 2 10^5 others
        one = np.concatenate([rng.uniform(1.2, 1.59, (100000, 3)), rng.uniform(-20, 20, (200000, 3))])
        return cloud(one[rng.permutation(one.shape[0])]), 0.4
    if name.startswith("threshold_"):
        return cloud(rng.uniform(-30, 30, (int(name.split("_")[1]), 3))), 0.4
    if name.startswith("tall_"):
        return tall_cloud(int(name.split("_")[1]), rng), 1.0
    assert name == "n1"
    return cloud(np.array([[1.0, -2.0, 3.0]])), 0.4


def _int_max_case(above):
    """a box of 1289.5 m: leaf 1 gives dx = dy = dz = 1290 (1290^3 < INT_MAX), a slightly smaller leaf 1291^3 > INT_MAX"""
    rng = np.random.default_rng(11)
    xyz = rng.uniform(0, 1289.5, (300000, 3)).astype(np.float32)
    xyz[0] = 0.0
    xyz[1] = 1289.5
    leaf = np.float32(0.9995 if above else 1.0)
    d = np.int64(np.float32(np.float32(1289.5) * (np.float32(1) / leaf))) + 1
    assert (d ** 3 > 2 ** 31 - 1) == above, d
    return np.concatenate([xyz, rng.uniform(0, 1, (300000, 1)).astype(np.float32)], axis=1), float(leaf)


@pytest.fixture(scope="module")
def vg_handle():
    h = binding.Handle(synth.default_params(16, 1800))
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", VG_CASES)
def test_voxel_grid_large(vg_handle, name):
    pts, leaf = _vg_case(name)
    want = _O().voxel_grid(pts, leaf, 0)
    assert_bit_equal(vg_handle.voxel_grid_large(pts, leaf), want, f"VoxelGrid {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("above", [False, True])
def test_voxel_grid_int_max_rule(vg_handle, above):
    pts, leaf = _int_max_case(above)
    got = vg_handle.voxel_grid_large(pts, leaf)
    want = _O().voxel_grid(pts, leaf, 0)
    assert_bit_equal(got, want, f"VoxelGrid at the INT_MAX rule (above={above})")
    if above:
        assert_bit_equal(got, pts, "pass-through keeps the input order")


@pytest.mark.gpu
def test_voxel_grid_device_path_on_small_clouds():
    """the multi-kernel path forced onto small clouds (empty, one point, one voxel, a few thousand points)"""
    h = binding.Handle(synth.default_params(16, 1800))
    h.set_option("ALEGO_GV_SMALL_MAX", 0)
    rng = np.random.default_rng(5)
    assert h.voxel_grid_large(np.zeros((0, 4), np.float32), 0.4).shape == (0, 4)
    for n in (1, 2, 7, 4095, 4097, 20000):
        pts = np.concatenate([rng.uniform(-5, 5, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
        assert_bit_equal(h.voxel_grid_large(pts, 0.4), _O().voxel_grid(pts, 0.4, 0), f"device path n={n}")
    pts = np.full((5000, 4), 0.1, np.float32)
    pts[:, 3] = rng.uniform(0, 1, 5000)
    assert_bit_equal(h.voxel_grid_large(pts, 0.4), _O().voxel_grid(pts, 0.4, 0), "one voxel")
    h.close()


@pytest.mark.gpu
def test_default_path_untouched():
    p = synth.default_params(16, 1800)
    h = binding.Handle(p)
    h.profile_enable(True)
    for k in range(6):
        h.scan_process(synth.scan(p, k), stages=7)
    names = list(h.profile_report())
    assert "lm_store_kf" in names
    assert not [n for n in names if n.startswith(("map_archive", "map_offsets", "map_gather", "gv_", "gs_"))], names
    L = binding.lib()
    st = np.zeros(4, np.int32)
    assert L.alego_map_status(h._h, 0, st.ctypes.data) == binding.ERR_ARG
    assert L.alego_map_assemble(h._h, 0, ALL, 0.0, None, 0) == binding.ERR_ARG
    assert L.alego_map_keyposes(h._h, 0, None, 0) == binding.ERR_ARG
    assert L.alego_map_set_keyposes(h._h, 0, 0, 0, None) == binding.ERR_ARG
    assert L.alego_map_enable(h._h, 16, 1000) == binding.ERR_ARG   # key frames exist already
    h.close()
    h = binding.Handle(p)
    assert L.alego_map_enable(h._h, 16, 1000) == 0
    assert L.alego_map_enable(h._h, 16, 1000) == binding.ERR_ARG   # once
    h.close()
    hs = binding.Handle(p, n_slots=3)
    hs.replay_create(1, 4)
    for k in range(4):
        hs.replay_load(0, k, synth.scan(p, k))
    hs.stream_setup(0)
    assert L.alego_map_enable(hs._h, 16, 1000) == binding.ERR_ARG
    hs.close()


@pytest.mark.gpu
def test_replay_save_map_matches_binding(tmp_path):
    exe = os.path.join(ROOT, "examples", "replay")
    r = subprocess.run([exe, "60", "--save-map", str(tmp_path), "--map-leaf", "0.4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    p = synth.default_params(16, 1800)
    h = binding.Handle(p)
    h.map_enable(4096, 1 << 24)
    for k in range(60):
        h.scan_process(synth.scan(p, k), stages=7, stamp=0.1 * k)
    want = {"keypose.pcd": h.map_keyposes(), "corner.pcd": h.map_assemble(binding.MAP_CORNER | binding.MAP_FRAME_ID),
            "surf.pcd": h.map_assemble(binding.MAP_SURF | binding.MAP_FRAME_ID), "outlier.pcd": h.map_assemble(binding.MAP_OUTLIER | binding.MAP_FRAME_ID),
            "global.pcd": h.map_assemble(ALL, 0.4)}
    assert want["keypose.pcd"].shape[0] >= 3
    for f, w in want.items():
        head, data = read_pcd(str(tmp_path / f))
        assert int(head["WIDTH"]) == w.shape[0], f
        assert_bit_equal(np.frombuffer(data, np.float32).reshape(-1, 4), w, f)
    h.close()
