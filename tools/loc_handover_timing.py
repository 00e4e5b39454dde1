"""Wall time of handing a slot's archive to a localising handle: the host route against the device route, same build.

  host    N x alego_map_get_keyframe (one call per frame into buffers of the handle's capacity, the clouds copied out as a host keeps
          them) + alego_loc_enable
  device  alego_loc_enable_from_map
on two archives: the synthetic lap's (mapped here, about 50 frames) and a constructed one of --frames frames of about --points points
(inserted with alego_lm_add_keyframe).  The routes alternate; every repetition uses a fresh localising handle, created and destroyed
outside the timed region; median and spread (max - min) of --reps repetitions.  The device route is also timed at chunk sizes 32 / 128 / 512
(ALEGO_LOC_CHUNK; the byte budget may clamp the largest), and alego_loc_update_from_map alone on a handle that already localises.  One JSON
line per archive.

    python tools/loc_handover_timing.py [--frames 2000] [--points 3000] [--reps 5] [--lap 560]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alego_loader import load_package  # noqa: E402

load_package()
from alego_amd import binding, synth  # noqa: E402

F32 = np.float32


def host_route(hm, hl, nf, radius, bufs):
    """seconds: the frames to the host, then alego_loc_enable"""
    L = binding.lib()
    t0 = time.perf_counter()
    kfs, keep = (binding.KfIn * max(nf, 1))(), []
    for i in range(nf):
        k = binding.KeyFrame()
        k.corner, k.corner_cap = bufs[0].ctypes.data, bufs[0].shape[0]
        k.surf, k.surf_cap = bufs[1].ctypes.data, bufs[1].shape[0]
        k.outlier, k.outlier_cap = bufs[2].ctypes.data, bufs[2].shape[0]
        rc = L.alego_map_get_keyframe(hm._h, 0, i, C.byref(k))
        assert rc >= 0, rc
        arrs = [bufs[0][:k.n_corner].copy(), bufs[1][:k.n_surf].copy(), bufs[2][:k.n_outlier].copy()]
        keep.append(arrs)
        kfs[i].pose[:] = k.pose[:]
        kfs[i].corner, kfs[i].n_corner = arrs[0].ctypes.data, k.n_corner
        kfs[i].surf, kfs[i].n_surf = arrs[1].ctypes.data, k.n_surf
        kfs[i].outlier, kfs[i].n_outlier = arrs[2].ctypes.data, k.n_outlier
    rc = L.alego_loc_enable(hl._h, kfs, nf, float(radius))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt


def device_route(hm, hl, radius, capacity=0):
    t0 = time.perf_counter()
    hl.loc_enable_from_map(hm, 0, radius, capacity)
    return time.perf_counter() - t0


def stats(v):
    return dict(ms=[round(1e3 * x, 3) for x in v], median=round(1e3 * float(np.median(v)), 3), spread=round(1e3 * (max(v) - min(v)), 3))


def measure(name, hm, p, reps, radius=6.0):
    nf, _, pts, _ = hm.map_status()
    bufs = [np.empty((hm.N, 4), F32) for _ in range(3)]
    row = dict(archive=name, frames=nf, points=pts)
    host, dev = [], []
    for r in range(reps + 1):   # (the first round warms both routes up and is dropped)
        for route in ("host", "device"):
            hl = binding.Handle(p)
            dt = host_route(hm, hl, nf, radius, bufs) if route == "host" else device_route(hm, hl, radius)
            hl.close()
            if r:
                (host if route == "host" else dev).append(dt)
    row["host"], row["device"] = stats(host), stats(dev)
    row["device_slowest_beats_host_fastest"] = bool(max(dev) < min(host))
    for c in (32, 128, 512):
        v = []
        for r in range(reps + 1):
            hl = binding.Handle(p)
            hl.set_option("ALEGO_LOC_CHUNK", c)
            dt = device_route(hm, hl, radius)
            hl.close()
            if r:
                v.append(dt)
        row[f"device_chunk_{c}"] = stats(v)
    hl = binding.Handle(p)
    hl.loc_enable_from_map(hm, 0, radius)
    v = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        hl.loc_update_from_map(hm, 0)
        if r:
            v.append(time.perf_counter() - t0)
    hl.close()
    row["update"] = stats(v)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lap", type=int, default=560)
    a = ap.parse_args()
    p = synth.default_params(16, 1800)
    pl = synth.default_params(16, 1800)
    pl.recent_keyframe_num = 10
    hm = binding.Handle(p)
    hm.map_enable(256, 1 << 20)
    for k in range(a.lap):
        hm.scan_process(synth.scan(p, k), stages=7)
    measure("lap", hm, pl, a.reps)
    hm.close()
    rng = np.random.default_rng(1)
    hm = binding.Handle(p)
    hm.map_enable(a.frames + 8, a.frames * (a.points + 64))
    nc, no = a.points // 6, a.points // 5
    ns = a.points - nc - no
    for i in range(a.frames):   # a lawn-mower path, 1 m between frames; clouds of a ring of walls around each pose
        pose = np.array([i % 100, (i // 100) * 5.0, 0.0, 0.0, 0.0, 0.1 * (i % 7)], F32)
        cl = lambda n: np.c_[rng.uniform(-30, 30, (n, 2)), rng.uniform(-2, 8, n), rng.uniform(0, 100, n)].astype(F32)
        hm.lm_add_keyframe(pose, cl(nc), cl(ns), cl(no))
    measure(f"constructed_{a.frames}x{a.points}", hm, pl, a.reps)
    hm.close()


if __name__ == "__main__":
    main()
