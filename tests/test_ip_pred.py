"""-m "not gpu": csrc/ip_pred.h — ImageProjection's ground test and edge predicate with their f32 screens — on the host.

tests/ip_pred/ip_pred_check.cpp asserts that whenever a screen decides, its answer is the full decision (the fp64 margins with their fall-through to the
reference's atan2 expression) and the site lies outside the fp64 margin band.  Edges: four (seg_alpha, seg_theta) sets, the defaults and a small
tan(theta) among them; d2 over 10000 f32 values from 0.3 m to 200 m with d1 at every f32 within 64 ulps of d2 K; 10^7 random pairs with ratios uniform
in [1, 1.05] (fewer than 1e-5 of a set's may stay undecided); d1 = d2; zero, denormal, infinite and NaN operands and theta outside (0, 1.5), which must all stay undecided.
Ground: slopes within 1e-5 (relative) of either bound at h from 1e-3 m to 1e2 m, zero, denormal, huge and non-finite differences, NaN tans.
Built with -ffp-contract=off (the device build's setting), AddressSanitizer and UBSan as a program of its own; the header must be readable by a host
compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_screens_equal_the_full_decisions_where_they_decide(tmp_path):
    exe = str(tmp_path / "ip_pred_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "ip_pred", "ip_pred_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "ip_pred ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
