"""The layout of the key-frame ring and of the key-frame archive at the shapes where offsets collapse: empty clouds, one point of one
kind, a ring of three rows that wraps, three slots in two stream groups.  Everything is inserted with alego_lm_add_keyframe and read back
bit for bit by both readers (ring: alego_lm_get_keyframe, archive: alego_map_get_keyframe) and by alego_map_assemble.

The poses have zero angles: keypose_matrix is then exactly [I | t] (cosf(0) = 1, sinf(0) = 0), and kf_transform gives
((1 * x + 0 * y) + 0 * z) + t = x + t in f32, which numpy computes with the same single addition."""
import ctypes as C

import numpy as np
import pytest

from alego_amd import binding
from util import assert_bit_equal

SIZES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 3, 1)]   # (corner, surf, outlier) of frames 0..4
SLOTS = (0, 2)
K = 2   # recent_keyframe_num: the ring has 3 rows, the 2 newest frames are resident


def _cloud(slot, f, kind, n):
    i = np.arange(n, dtype=np.float32)
    x = np.float32(1000 * slot + 100 * f + 10 * kind) + i + np.float32(0.25)
    return np.stack([x, -x * np.float32(0.5), x * np.float32(0.25) + np.float32(0.5), np.float32(7000) + x], axis=1).astype(np.float32)


def _pose(slot, f):
    return np.array([3.5 + f + 20 * slot, -1.25 * (f + 1) - slot, 0.125 * (f + 2) + 2 * slot, 0, 0, 0], np.float32)


def _frames(slot):
    return [dict(pose=_pose(slot, f), corner=_cloud(slot, f, 0, nc), surf=_cloud(slot, f, 1, ns), outlier=_cloud(slot, f, 2, no))
            for f, (nc, ns, no) in enumerate(SIZES)]


def _same_frame(got, want, f, tag):
    assert got["id"] == f, tag
    assert_bit_equal(got["pose"], want["pose"], f"{tag}: pose")
    for kind in ("corner", "surf", "outlier"):
        assert got[kind].shape == want[kind].shape, f"{tag}: {kind} count"
        assert_bit_equal(got[kind], want[kind], f"{tag}: {kind} cloud")


def _map(frames, kinds):
    """frames in id order, surf then corner then outlier inside a frame, p + t, intensity = frame id under MAP_FRAME_ID"""
    parts = [np.zeros((0, 4), np.float32)]
    for f, fr in enumerate(frames):
        for bit, kind in ((binding.MAP_SURF, "surf"), (binding.MAP_CORNER, "corner"), (binding.MAP_OUTLIER, "outlier")):
            if kinds & bit:
                t = fr[kind].copy()
                t[:, :3] = t[:, :3] + fr["pose"][:3]
                if kinds & binding.MAP_FRAME_ID:
                    t[:, 3] = np.float32(f)
                parts.append(t)
    return np.concatenate(parts)


def _check_slot(h, slot, frames, tag):
    n = len(frames)
    assert h.lm_keyframe_count(slot) == n and h.map_status(slot)[:3] == (n, 0, sum(sum(s) for s in SIZES)), tag
    for f in range(n - K, n):
        _same_frame(h.lm_get_keyframe(f, slot=slot), frames[f], f, f"{tag}: ring frame {f}")
    _same_frame(h.lm_get_keyframe(-1, slot=slot), frames[n - 1], n - 1, f"{tag}: newest ring frame")
    for f in range(n):
        _same_frame(h.map_get_keyframe(f, slot=slot), frames[f], f, f"{tag}: archived frame {f}")
    for kinds in (1, 2, 4, 7, 7 | 8):
        assert_bit_equal(h.map_assemble(kinds, 0.0, slot=slot), _map(frames, kinds), f"{tag}: map kinds {kinds}")
    assert_bit_equal(h.map_assemble(7, -1.0, slot=slot), _map(frames, 7), f"{tag}: map kinds 7, negative leaf")


def _slot1_empty(h):
    assert h.lm_keyframe_count(1) == 0
    assert h.map_status(1)[:3] == (0, 0, 0)
    assert h.map_assemble(7, 0.0, slot=1).shape == (0, 4)


def _reader_calls(h, slot, f):
    L = binding.lib()
    return (("alego_lm_get_keyframe", lambda k: L.alego_lm_get_keyframe(h._h, slot, f, C.byref(k))),
            ("alego_map_get_keyframe", lambda k: L.alego_map_get_keyframe(h._h, slot, f, C.byref(k))))


@pytest.mark.gpu
def test_ring_and_archive_layout_at_collapsing_offsets(params_a, monkeypatch):
    p = params_a.copy()
    p.recent_keyframe_num = K
    monkeypatch.setenv("ALEGO_STREAM_GROUPS", "2")   # slots 0 and 1 share a stream group, slot 2 is alone in the second
    h = binding.Handle(p, n_slots=3, ring_len=1)
    monkeypatch.delenv("ALEGO_STREAM_GROUPS")
    assert h.stream_groups() == (2, 2)
    h.map_enable(8, 64)
    want = {s: _frames(s) for s in SLOTS}
    for f in range(len(SIZES)):
        for s in SLOTS:
            fr = want[s][f]
            h.lm_add_keyframe(fr["pose"], fr["corner"], fr["surf"], fr["outlier"], slot=s)
        _slot1_empty(h)
    for s in SLOTS:
        _check_slot(h, s, want[s], f"slot {s}")
        for f in (len(SIZES) - K - 1, len(SIZES), 0):   # the frame the window dropped last, a frame that does not exist yet, the oldest
            with pytest.raises(binding.AlegoError):
                h.lm_get_keyframe(f, slot=s)
        with pytest.raises(binding.AlegoError):
            h.map_get_keyframe(len(SIZES), slot=s)
    _slot1_empty(h)

    # the count-only form, and buffers one point too small
    last = len(SIZES) - 1
    for s in SLOTS:
        for f in (last - 1, last):
            for name, call in _reader_calls(h, s, f):
                k = binding.KeyFrame()
                assert call(k) == 0, name
                assert (k.id, k.n_corner, k.n_surf, k.n_outlier) == (f,) + SIZES[f], f"{name}: slot {s} frame {f} counts"
                assert_bit_equal(np.array(k.pose[:], np.float32), want[s][f]["pose"], f"{name}: slot {s} frame {f} pose")
        for name, call in _reader_calls(h, s, last):
            for short in range(3):
                bufs = [np.full((4, 4), -1, np.float32) for _ in range(3)]
                caps = [n - 1 if i == short else n for i, n in enumerate(SIZES[last])]
                k = binding.KeyFrame()
                k.corner, k.corner_cap = bufs[0].ctypes.data, caps[0]
                k.surf, k.surf_cap = bufs[1].ctypes.data, caps[1]
                k.outlier, k.outlier_cap = bufs[2].ctypes.data, caps[2]
                assert call(k) == binding.ERR_CAPACITY, f"{name}: slot {s}, buffer {short} one point too small"
                assert (k.n_corner, k.n_surf, k.n_outlier) == SIZES[last], name
                for b in bufs:
                    assert np.all(b == -1), f"{name}: wrote into a buffer it refused"

    # a new pose for a resident frame of slot 2: both readers and the map follow, slot 0 keeps everything
    for f in (last, last - 1):
        new = np.array([-40.5 - f, 17.25 + f, 2.75 * f, 0, 0, 0], np.float32)
        h.lm_set_keypose(f, new, slot=2)
        want[2][f] = dict(want[2][f], pose=new)
        _check_slot(h, 2, want[2], f"slot 2 after set_keypose({f})")
        _check_slot(h, 0, want[0], f"slot 0 after slot 2's set_keypose({f})")
        _slot1_empty(h)
    with pytest.raises(binding.AlegoError):
        h.lm_set_keypose(last - K, want[2][0]["pose"], slot=2)   # not resident
    h.close()


@pytest.mark.gpu
def test_a_frame_with_a_negative_count_is_refused(params_a):
    """alego_loop_closure_icp, alego_lm_add_keyframe and alego_loc_enable: ALEGO_ERR_ARG for a negative count or a missing cloud, whichever
    cloud it is and whichever frame of the list"""
    L = binding.lib()
    h = binding.Handle(params_a)
    pts = np.zeros((4, 4), np.float32)
    pts[:, 0] = np.arange(4)

    def kf(n_corner=2, n_surf=2, n_outlier=2, null=None):
        k = binding.KfIn()
        k.pose[:] = [0.0] * 6
        k.corner, k.n_corner = (None if null == 0 else pts.ctypes.data), n_corner
        k.surf, k.n_surf = (None if null == 1 else pts.ctypes.data), n_surf
        k.outlier, k.n_outlier = (None if null == 2 else pts.ctypes.data), n_outlier
        return k

    bad = [kf(n_corner=-1), kf(n_surf=-1), kf(n_outlier=-1), kf(null=0), kf(null=1), kf(null=2)]
    out = binding.IcpResult()
    pose = np.zeros(6, np.float32)
    for i, b in enumerate(bad):
        good = kf()
        assert L.alego_loop_closure_icp(h._h, C.byref(b), None, 0, C.byref(out), None, 0) == binding.ERR_ARG, f"loop closure: newest frame, case {i}"
        hist = (binding.KfIn * 2)(good, b)
        assert L.alego_loop_closure_icp(h._h, C.byref(good), hist, 2, C.byref(out), None, 0) == binding.ERR_ARG, f"loop closure: history frame, case {i}"
        assert L.alego_lm_add_keyframe(h._h, 0, pose.ctypes.data, b.corner, b.n_corner, b.surf, b.n_surf, b.outlier, b.n_outlier) == binding.ERR_ARG, f"add_keyframe: case {i}"
        assert h.lm_keyframe_count() == 0
        frames = (binding.KfIn * 2)(good, b)
        assert L.alego_loc_enable(h._h, frames, 2, 0.0) == binding.ERR_ARG, f"loc_enable: case {i}"
    # the handle is still the SLAM handle it was: the same frames without the bad one are taken
    good = kf()
    assert L.alego_lm_add_keyframe(h._h, 0, pose.ctypes.data, good.corner, 2, good.surf, 2, good.outlier, 2) == 0
    assert h.lm_keyframe_count() == 1
    h.close()
