"""-m "not gpu": csrc/fe_rules.h — the pick rules of feature extraction that every kernel path shares — on the host.

tests/fe_rules/fe_rules_check.cpp asserts, against the reference's loops (laserOdometry.cpp:122-285) written out plainly in the test:
  sectors     both sector formulas for n_sectors 1..9 and 24, rings from "no point" (E = S - 10) up to 80 points at five ring starts; the six-sector fast
              path against the general form (a divisor the compiler cannot see); sectors contiguous, tiling [S, E - 1]; which are skipped
  sums/marks  the 11-tap sum against a chain of volatile f32 partial sums, the key's order against the curvature's, the thresholds, the occlusion marks
              A / B / C in both occl_f32 modes on ranges either side of every limit, the column jump
  picked      the lane-mask form of "a point is picked" against the per-point form and the rule, on random marks over five 64-point chunks
  flags       the flag byte's predicates for all 256 bytes, fe_flag_of / fe_flag_with_label / fe_flag_label round trips, less_flat_scan membership
  reach       fe_reach (and the forms ff_span uses) against the reference's two loops for all 32 x 32 jump patterns and radius 0..5
  labels      fe_pick_label for all 0 <= n_sharp <= n_less_sharp <= 4, n_flat 1..4 over the first 8 picks: the (n_less_sharp + 1)-th pick is marked but not
              labelled and ends the loop, the n_flat-th pick ends the loop before the suppression
  rings       6000 random rings of up to 40 points with few distinct curvatures: a greedy best-remaining pick built from the header's rules alone gives
              the same four lists, labels and picked bits as sort-then-scan (stable sort = the (curvature, index) order of sort_mode 0); the tie rules
              of sort_mode 2 on their codes
Built with -ffp-contract=off (the device build's setting), AddressSanitizer and UBSan as a program of its own: nothing is preloaded, and the header must be
readable by a host compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_equal_the_reference_loops_written_out(tmp_path):
    exe = str(tmp_path / "fe_rules_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "fe_rules", "fe_rules_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fe_rules ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
