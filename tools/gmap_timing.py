"""Device times of the global-map path: map assembly + VoxelGrid at 1 M and 4 M points (leaf 0.4), the same
VoxelGrid on the one-workgroup kernel (vox_big) and the dispatch-threshold sweep of alego_voxel_grid.

Every number is the median over --reps calls of the summed HIP-event times of the call's kernels (alego_profile_*), so host copies
and synchronisation are not in it.

    python tools/gmap_timing.py [--reps 7] [--sizes 1048576,4194304] [--sweep 16384,32768,65536,131072,262144,524288]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alego_loader import load_package  # noqa: E402

load_package()
from alego_amd import binding, synth  # noqa: E402

ALL = binding.MAP_SURF | binding.MAP_CORNER | binding.MAP_OUTLIER


def device_ms(h, fn, reps):
    """median over reps of the summed kernel times of one call of fn()"""
    t = []
    for _ in range(reps):
        h.profile_enable(True)
        fn()
        rep = h.profile_report()
        h.profile_enable(False)
        t.append(sum(ms for ms, _ in rep.values()))
    return float(np.median(t))


def cloud(rng, n, clustered):
    if clustered:
        c = rng.uniform(-80, 80, (200, 3))
        xyz = c[rng.integers(0, 200, n)] + rng.normal(0, 2.0, (n, 3))
    else:
        xyz = rng.uniform(-100, 100, (n, 3))
    return np.concatenate([xyz, rng.uniform(0, 100, (n, 1))], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1048576,4194304")
    ap.add_argument("--sweep", default="16384,32768,65536,131072,262144,524288")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    p = synth.default_params(16, 1800)
    res = {"assemble_voxel": {}, "voxel_device": {}, "voxel_vox_big": {}, "sweep": {}}
    for n in [int(v) for v in a.sizes.split(",") if v]:
        # an archive of n points: frames of 14 k surf points inserted as key frames (the window is reset before each insertion)
        h = binding.Handle(p)
        h.map_enable(n // 14000 + 2, n)
        pts = cloud(rng, n, clustered=False) * np.float32(0.5)
        per = 14000
        for f in range(n // per):
            h.lm_reset_window()
            h.lm_add_keyframe(np.array([0.3 * f, 0.1 * f, 0, 0, 0, 0.01 * f], np.float32), pts[:0], pts[f * per:(f + 1) * per], pts[:0])
        m = h.map_status()[2]
        res["assemble_voxel"][m] = device_ms(h, lambda: h.map_assemble(ALL, 0.4), a.reps)
        res["assemble_only"] = res.get("assemble_only", {})
        res["assemble_only"][m] = device_ms(h, lambda: h.map_assemble(ALL, 0.0), a.reps)
        h.close()
        for clustered in (False, True):
            c = cloud(rng, n, clustered)
            key = f"{n}{'_clustered' if clustered else '_uniform'}"
            h = binding.Handle(p)
            res["voxel_device"][key] = device_ms(h, lambda: h.voxel_grid_large(c, 0.4), a.reps)
            h.set_option("ALEGO_GV_SMALL_MAX", 1 << 30)   # everything to one workgroup
            res["voxel_vox_big"][key] = device_ms(h, lambda: h.voxel_grid_large(c, 0.4), a.reps)
            h.close()
    for n in [int(v) for v in a.sweep.split(",") if v]:
        c = cloud(rng, n, clustered=True)
        h = binding.Handle(p)
        h.set_option("ALEGO_GV_SMALL_MAX", 0)
        dev = device_ms(h, lambda: h.voxel_grid_large(c, 0.4), a.reps)
        h.set_option("ALEGO_GV_SMALL_MAX", 1 << 30)
        one = device_ms(h, lambda: h.voxel_grid_large(c, 0.4), a.reps)
        res["sweep"][n] = {"device_ms": dev, "one_workgroup_ms": one}
        h.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
