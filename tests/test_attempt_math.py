"""-m "not gpu": csrc/reloc_math.h — the candidate word of the descriptor searches and the window of an ICP attempt, the two rules that kernels and
host code of alego_loop_search, the appearance search and relocalisation share — on the host.

tests/attempt_math/attempt_math_check.cpp compares them with values written out there and is built here with AddressSanitizer and UBSan as a
program of its own; the header must be readable by a host compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_candidate_word_and_attempt_window(tmp_path):
    exe = str(tmp_path / "attempt_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "attempt_math", "attempt_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "attempt_math ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
