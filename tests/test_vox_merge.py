"""-m "not gpu": csrc/vox_merge.h — the rules of lm_total_merge (laser_surf_total_ds_ as a stable merge of laser_surf_ds_ with the few points of
laser_outlier_ds_, and VoxelGrid of a small cloud by rank-by-counting) — on the host.

tests/vox_merge/vox_merge_check.cpp applies the header the way the kernel does and compares it bit for bit with a plain restatement of
pcl::VoxelGrid: bounding box, leaf-too-small rule, box-relative voxel ids in wrapping int arithmetic, std::stable_sort of S ++ O by id, sums from
0.f in that order divided by (float)count.  The filtered cloud in the form the kernel computes it (no merged cloud: a voxel's run = an S run followed by the O elements
of its key, found with vm_count_less / vm_count_le; its rank = the S heads and O-only voxels before it) and the counted filter are compared, and every
refusal must be one the plain statement predicts (S's cells out of lexicographic order, more than LT_OCAP outliers, a cell outside the key range,
the leaf-too-small rule, 2^32 cells, a NaN).  600 random S / O pairs built by the plain filter from raw clouds (half of them on a 0.05 m lattice,
whose points sit on cell boundaries; outlier leaf 1.0 and 0.8): the refuse rate is printed and may not exceed 1 %, and more than half of the pairs
must have a voxel that several points of S ++ O share.  Built cases: three points at 5.5999994f / -1.6000001f (and the opposite signs) whose f32
centroid lands in the next 0.8 m cell, alone, with an outlier in the old and in the new cell, into an occupied neighbour (must merge) and backwards
in the order (must refuse); an unsorted S; -0.f coordinates (a lone -0.f comes out +0.f); outliers before, after and between S's keys, several in
one voxel with and without a surf point; empty S, empty O, both; LT_OCAP and LT_OCAP + 1 outliers; cells beyond +-2^20; the leaf-too-small rule.
Built with -ffp-contract=off (the device build's setting), AddressSanitizer and UBSan as a program of its own; the headers must be readable by a
host compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_and_counted_filter_equal_the_plain_voxel_grid(tmp_path):
    exe = str(tmp_path / "vox_merge_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "vox_merge", "vox_merge_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "vox_merge ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
