"""The layout of the front end's per-slot device arrays (csrc/fe_store.h) where offsets collapse or a wrong stride reaches a neighbour: one ring,
odd ring counts on both sides of the banded path's threshold, three slots in two stream groups with an empty stream between two different ones, and
three scans so that each feature buffer is written and the double-buffer parity flips twice.

After every scan each front-end name alego_debug_get serves is read per slot and compared bit for bit with a one-slot handle fed the same stream
through alego_scan_process (there every slot offset is zero), and, for the names the oracle has, with the oracle stepped alongside.

Seven of the names are written only by a launch that covers ONE slot (launch_ip's keep_images, fe_front's and fe_pickc's `n_launch == 1`): the images
(range, labels, flags, owner, parent), curv_d and point_label, all plain [slot][N] arrays.  A launch of several slots leaves them as they were, so
they are compared for slot 2, which is alone in its stream group, against its one-slot handle and against the oracle; every other name is compared
for every slot."""
import numpy as np
import pytest

from alego_amd import binding, synth
from oracle import oracle_py as O
from util import assert_bit_equal

GEOMS = [(1, 512), (3, 720), (16, 100), (17, 70)]   # (17, 70) takes the banded path
STREAMS = {0: 0, 2: 1}                                # slot -> synthetic stream; slot 1 gets empty scans
NSCAN = 3
ONE_SLOT_ONLY = ("range_img", "label_img", "flag_img", "owner", "parent", "curv_d", "point_label")   # written only by a launch of one slot: slot 2 here
ALONE = 2
NAMES = ("seg_cloud", "seg_ground", "seg_col", "seg_range", "outlier", "ring_start", "ring_end",
         "orientation", "scal", "sharp", "less_sharp", "flat", "less_flat", "sharp_idx", "less_sharp_idx", "flat_idx",
         "lo_surf_corr", "lo_corner_corr", "lo_state", "poses")
ORACLE_WHOLE = ("seg_cloud", "seg_ground", "seg_col", "seg_range", "outlier", "ring_start", "ring_end", "orientation",
                "sharp", "less_sharp", "flat", "less_flat", "sharp_idx", "less_sharp_idx", "flat_idx")
ORACLE_ALONE = ("range_img",)                        # of ONE_SLOT_ONLY the oracle has these whole ...
ORACLE_INNER = ("curv_d", "point_label")              # ... and these for the points [5, M - 5) (as tests/test_gpu_parity.py compares them)
# (no entry of `scal` differs between alego_batch_run and alego_scan_process: the array is compared whole)
EMPTY = np.zeros((0, 4), np.float32)


def _scan(p, slot, k):
    return synth.scan(p, k, stream=STREAMS[slot]) if slot in STREAMS else EMPTY


def _same_pose(got, want, tag):
    assert got[0] == want[0], f"{tag}: flags"
    for a, b, which in ((got[1], want[1], "odom"), (got[2], want[2], "map")):
        assert a["valid"] == b["valid"], f"{tag}: {which} valid"
        for key in ("t", "q", "params"):
            assert_bit_equal(a[key], b[key], f"{tag}: {which} {key}")


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_slots_of_a_batch_match_one_slot_handles(geom, monkeypatch):
    p = synth.default_params(*geom)
    cap = p.n_scan * p.horizon_scan * 16 + 4096
    monkeypatch.setenv("ALEGO_STREAM_GROUPS", "2")   # slots 0 and 1 share a stream group, slot 2 is alone in the second
    hb = binding.Handle(p, n_slots=3, ring_len=NSCAN)
    monkeypatch.delenv("ALEGO_STREAM_GROUPS")
    assert hb.stream_groups() == (2, 2)
    ones = [binding.Handle(p) for _ in range(3)]
    oracles = {s: O.Oracle(p) for s in STREAMS}
    for s in range(3):
        for k in range(NSCAN):
            hb.batch_load(s, k, _scan(p, s, k))
    for k in range(NSCAN):
        hb.batch_run(k, 1, stages=3)
        for s in range(3):
            tag = f"{geom} scan {k} slot {s}"
            ones[s].scan_process(_scan(p, s, k), stages=3)
            for name in (ONE_SLOT_ONLY if s == ALONE else ()) + NAMES:
                assert_bit_equal(hb.debug_get(name, slot=s, cap_bytes=cap), ones[s].debug_get(name, cap_bytes=cap), f"{tag}: {name} against the one-slot handle")
            counts = hb.batch_get_counts(s)
            assert counts == ones[s].batch_get_counts(), f"{tag}: counts"
            _same_pose(hb.batch_get_pose(s), ones[s].batch_get_pose(), tag)
            if s in STREAMS:
                o = oracles[s]
                o.process_scan(_scan(p, s, k))
                m = o.get("seg_cloud").shape[0]
                for name in ORACLE_WHOLE + (ORACLE_ALONE if s == ALONE else ()):
                    assert_bit_equal(hb.debug_get(name, slot=s, cap_bytes=cap), o.get(name), f"{tag}: {name} against the oracle")
                for name in ORACLE_INNER if s == ALONE else ():
                    assert_bit_equal(hb.debug_get(name, slot=s, cap_bytes=cap)[5:m - 5], o.get(name)[5:m - 5], f"{tag}: {name} against the oracle")
            else:   # the empty stream between them: no count, no cloud, whatever its neighbours hold
                assert [counts[c] for c in ("P", "M", "O", "Qc", "Fc", "Qs", "Fs", "n_surf_corr", "n_corner_corr")] == [0] * 9, f"{tag}: counts {counts}"
                for name in ("seg_cloud", "outlier", "sharp", "less_sharp", "flat", "less_flat"):
                    assert hb.debug_get(name, slot=s, cap_bytes=cap).shape == (0, 4), f"{tag}: {name} is not empty"
    for h in ones + [hb]:
        h.close()
