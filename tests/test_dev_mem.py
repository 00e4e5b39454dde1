"""-m "not gpu": csrc/dev_mem.h — DevPool and DevBuf, the host side's one owner of device memory — on the host heap.

tests/dev_mem/dev_mem_check.cpp supplies guard_alloc.h's functions as stubs (live-block count, non-zero fill, failure of the k-th request) and is
built here with AddressSanitizer and UBSan as a program of its own: a leak, a double free or a write past a block ends it with a non-zero status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_mem_owns_and_frees_every_block_once(tmp_path):
    exe = str(tmp_path / "dev_mem_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"),
           os.path.join(ROOT, "tests", "dev_mem", "dev_mem_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "dev_mem ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
