"""-m "not gpu": csrc/dev_copy.h — the host side's one definition of copies between host and device and of waits — on the host heap.

tests/dev_copy/dev_copy_check.cpp supplies hipMemcpy, hipMemcpyAsync, hipStreamSynchronize and hipGetErrorString as stubs (memcpy, a record of every
call's byte count, kind and stream, failure of the k-th call) and is built here with AddressSanitizer and UBSan as a program of its own, not linked
against the HIP runtime: a copy that is one byte too long for its exactly sized buffer ends it with a non-zero status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_copy_counts_bytes_and_keeps_the_first_error(tmp_path):
    exe = str(tmp_path / "dev_copy_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"),
           os.path.join(ROOT, "tests", "dev_copy", "dev_copy_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "dev_copy ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
