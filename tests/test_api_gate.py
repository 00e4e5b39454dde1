"""-m "not gpu": csrc/api_gate.h — the list rules every batched entry point of the C ABI shares — on the host.

tests/api_gate/api_gate_check.cpp states each rule plainly (a walk over the list with a nested loop instead of the header's tables) and compares the
header's code and exact message with it, and with the expectation written out for every case:
  slot lists   n = 0 with a null list; n_slots = 1; slots -1, n_slots, INT_MIN, INT_MAX; a duplicate adjacent, and as first and last entry; the same
               lists with `distinct` off (accepted); all n_slots slots in reverse order; two faults in one list: the first offender in list order is named
  pair lists   a self pair; either side out of range; (a, b) twice against (a, b), (b, a) for the align rule; for the merge rule a destination listed
               twice, a destination that is also a source, a source listed twice (legal); the order in which two faults are reported
A list that passes leaves the message string untouched.  Built with AddressSanitizer and UBSan as a program of its own: nothing is preloaded, and the
header must be readable by a host compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_rules_equal_their_plain_statements(tmp_path):
    exe = str(tmp_path / "api_gate_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "api_gate", "api_gate_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "api_gate ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
