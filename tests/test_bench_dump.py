"""bench.py --dump-outputs: what the timed steps computed, as float32 / float64 .npy files that two runs (or two builds) can be compared by."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alego_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _FakeHandle:
    """batch_get_pose / debug_get of a handle whose slot 3 reports an error and whose surf map is larger than bench.DUMP_ROWS"""

    def batch_get_pose(self, s):
        if s == 3:
            raise binding.AlegoError("capacity")
        pose = dict(t=np.arange(3.0) + s, q=np.array([1.0, 0, 0, 0]), params=np.full(6, 0.5 * s), valid=1)
        return s % 7, pose, dict(pose)

    def debug_get(self, name, slot=0):
        rng = np.random.default_rng(slot)
        if name == "seg_col":
            return rng.integers(0, 1800, 1000).astype(np.int32)
        return rng.random((3 * bench.DUMP_ROWS if name == "lm_surf_map_ds" else 500, 4), dtype=np.float32)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_float_bounded_and_repeatable(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(_FakeHandle(), 64, str(a))
    bench.dump_outputs(_FakeHandle(), 64, str(b))
    da, db = _load(a), _load(b)
    assert da.keys() == db.keys()
    assert all(np.array_equal(da[k], db[k], equal_nan=True) for k in da)
    assert all(v.dtype in (np.float32, np.float64) for v in da.values())
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_BUDGET
    slots = da["cloud_slots"].astype(int)
    assert len(slots) == bench.DUMP_SLOTS and all(f"slot{s}_{n}" in da for s in slots for n in bench.CHECK_ARRAYS)
    assert max(v.shape[0] for v in da.values()) == bench.DUMP_ROWS          # the large cloud is sampled down
    assert da["flags"][3] == -1 and np.isnan(da["odom_t"][3]).all()        # the slot that reported an error
    assert da["flags"][5] == 5 and np.array_equal(da["map_params"][5], np.full(6, 2.5))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--streams", "64", "--bags", "1", "--prime", "20",
           "--no-cpu", "--no-check", "--no-isolated", "--no-profile", "--no-configs", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_repeats_run_to_run(tmp_path):
    ja, jb = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    assert ja["steps"] == jb["steps"] == 3 and ja["ms_per_step"] > 0 and jb["ms_per_step"] > 0
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert da.keys() == db.keys() and da["odom_t"].shape == (64, 3)
    assert not np.isnan(da["map_t"]).any()
    diff = [k for k in da if not np.array_equal(da[k].view(np.uint8), db[k].view(np.uint8))]
    assert not diff, diff
