"""-m "not gpu": csrc/solve_rows.h — the cost functors and the trust-region control the two solvers share — on the host.

tests/solve_rows/solve_rows_check.cpp runs the cost-only evaluation of a candidate against the cost the full evaluation delivers, the accumulators of
LaserOdometry's non-zero Jacobian columns against the generic 28 sums (rows for the non-finite guard included), and whole solves
with the cost-first control (both candidate policies, and its FULL_EVAL mode) against the solver that evaluates every point in full, bit for bit.
It is built here with -ffp-contract=off (the device build's setting), AddressSanitizer and UBSan as a program of its own; the header must be
readable by a host compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cost_first_control_equals_full_evaluation(tmp_path):
    exe = str(tmp_path / "solve_rows_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "solve_rows", "solve_rows_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "solve_rows ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
