"""-m "not gpu": csrc/ip_rules.h — the output rules of ImageProjection that every kernel path shares — on the host.

tests/ip_rules/ip_rules_check.cpp asserts that the row-mask forms (16 rows in a uint32_t: NS 1, 2, 5, 16; 64 rows in a uint64_t: NS 17, 40, 64) equal the
per-cell form bit for bit, and that the per-cell form equals the rule written out in the test as a plain double loop over the image, for H in 1, 4, 5, 6,
9, 10, 11, 64, 70, every column of every H and ground_scan_id in -5, -1, 0, 1, NS - 2, NS - 1, NS, NS + 5, INT_MAX.  Column states (ground and active
disjoint, feasible within active): all of them up to NS = 5, at every column and ground id; 10^5 random ones for each larger NS, each at every ground id and
at one column, the columns of all H taken in turn (a column enters the mask forms through ip_ground_col_kept / ip_outlier_col alone, which the per-cell
form calls too and the double loop checks at every column).  ip_seg_feasible at 4, 5, 29, 30 cells over 2 and 3 rows.
Built with -ffp-contract=off (the device build's setting), AddressSanitizer and UBSan as a program of its own: no shift count of the header leaves its
type, and the header must be readable by a host compiler without the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_forms_equal_the_cell_form_and_the_cell_form_the_rule(tmp_path):
    exe = str(tmp_path / "ip_rules_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "ip_rules", "ip_rules_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "ip_rules ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
