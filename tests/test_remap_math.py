"""-m "not gpu": csrc/remap_math.h and the projected lm_step of csrc/solve_rows.h — solution remapping of LaserMapping's registration (DESIGN.md
section 23) — on the host.

tests/remap_math/remap_math_check.cpp is built here with AddressSanitizer and UBSan as a program of its own (the headers must be readable by a
host compiler without the HIP runtime): projector identities, every status, lm_step with no projector against the plain lm_step, whole solves
under the projection in every candidate policy bit for bit, and the shift along every held direction.

The host twins alego_remap_host + alego_remap_step_host are then compared through the binding with tests/remap_ref.py (numpy.linalg.eigh, the
explicitly inverted M, numpy's Cholesky) on the constructed cases.  Tolerances: the largest deviation from numpy measured over CASES —
eigenvalues relative to lambda_max, proj to its largest entry, a step to its largest entry, the model cost change to itself — and 16 x that
asserted (the project's convention, tests/test_reg_cov_math.py):
    measured   eigenvalues 4.06e-15   proj 5.22e-15   step 6.84e-15   mcc 3.19e-15
    asserted   (16 x)      6.50e-14        8.35e-14        1.09e-13       5.10e-14
(Each side starts from its own normal equations — alego_regcov_normal_host against stacked numpy Jacobians, section 22 — then numpy's eigh stands
against the cyclic Jacobi, its inverse of M against the closed form, its Cholesky against the solver's.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import regcov_ref as ref
import remap_ref as rr
from alego_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_remap_enable", "alego_remap_get", "alego_remap_host", "alego_remap_step_host", "alego_debug_remap_solve"]
TOL = dict(eigval=6.50e-14, proj=8.35e-14, step=1.09e-13, mcc=5.10e-14)   # 16 x the measured figures of the header


def test_math_headers_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "remap_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "remap_math", "remap_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "remap_math ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_header_library_and_binding_have_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(binding.lib(), s) and s in binding.EXPORTS, s
    assert C.sizeof(binding.Remap) == 16 + 8 * 84 and C.sizeof(binding.RemapOpts) == 8


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_constructed_cases_are_what_they_claim(name):
    """numpy alone: the held count, no eigenvalue within 1e-3 of eig_min; the plain restatement moves more than 0.1 m along the held direction of a
    spurious corridor and the projected one does not move along it"""
    rec, moved = rr.check_preconditions(name)
    x0, E, S, eig_min, held = rr.CASES[name]
    f = rr.frame(x0, E, S, True, eig_min)
    shift = rr.held_shift(rec, f["params_it"][1])
    print(f"{name}: eigenvalues {rec['eigval'][:3]}, held {rec['n_held']}, plain shift {moved}, projected shift {shift}, iterations {f['iterations']}, termination {f['termination']}")
    assert np.all(np.abs(shift) < 1e-12)
    if held == 6:
        assert np.array_equal(f["params_it"], np.tile(x0, (2, 1))) and list(f["termination"]) == [2, 2]
    if held == 0:
        g = rr.frame(x0, E, S, False, eig_min)
        assert np.array_equal(f["params_it"], g["params_it"])


def deviations(got, want):
    f = dict(eigval=0.0, proj=0.0)
    if want["status"] == 1:
        f["eigval"] = np.abs(got["eigval"] - want["eigval"]).max() / np.abs(want["eigval"]).max()
        f["proj"] = np.abs(got["proj"] - want["proj"]).max() / max(np.abs(want["proj"]).max(), 1.0)
    return f


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_host_twins_against_numpy(name):
    x0, E, S, eig_min, held = rr.CASES[name]
    want_acc = ref.normal_equations(x0, E, S)
    want = rr.projector(want_acc, x0, len(E), len(S), eig_min)
    acc = binding.regcov_normal_host(x0, E, S, ref.HUBER)
    got = binding.remap_host(acc, x0, len(E), len(S), binding.remap_opts(eig_min))
    assert got["status"] == want["status"] == 1 and got["n_held"] == want["n_held"] == held and got["frame"] == 0
    assert np.array_equal(got["start"], x0)
    f = deviations(got, want)
    if held == 0:
        assert np.array_equal(got["proj"], np.eye(6))
    if held == 6:
        assert not np.any(got["proj"])
    # the first step of the solve, plain and projected, from the twin's own normal equations
    scale = 1.0 / (1.0 + np.sqrt(np.array([acc[k] for k in (0, 6, 11, 15, 18, 20)])))
    f["step"], f["mcc"] = 0.0, 0.0
    for proj_g, proj_w in ((None, None), (got["proj"], want["proj"])):
        ok_g, st_g, mcc_g = binding.remap_step_host(acc[:21], acc[21:27], scale, 1e4, proj_g)
        ok_w, st_w, mcc_w, null = rr.step(want_acc[:21], want_acc[21:27], scale, 1e4, proj_w)
        assert ok_g == ok_w
        if null:
            assert not np.any(st_g) and mcc_g == 0.0
        else:
            f["step"] = max(f["step"], np.abs(st_g - st_w).max() / np.abs(st_w).max())
            f["mcc"] = max(f["mcc"], abs(mcc_g - mcc_w) / abs(mcc_w))
    print(f"{name}: deviation from numpy " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
    for k, v in f.items():
        assert v <= TOL[k], (name, k, v, TOL[k])
    # the projected step keeps the held directions: M0 dx . v_held at rounding level of the step
    if 0 < held < 6:
        _, st, _ = binding.remap_step_host(acc[:21], acc[21:27], scale, 1e4, got["proj"])
        xi = want["M"] @ st
        assert np.abs(got["eigvec"][:, :held].T @ xi).max() <= 1e-13 * max(np.abs(st).max(), 1.0)


def test_statuses_and_options_through_the_binding():
    x0, E, S, eig_min, _ = rr.CASES["courtyard_100"]
    acc = binding.regcov_normal_host(x0, E, S, ref.HUBER)
    assert binding.remap_host(acc, x0, len(E), len(S))["n_held"] == 2                     # NULL options: eig_min 100
    assert binding.remap_host(acc, x0, len(E), len(S), binding.remap_opts(-5.0))["n_held"] == 2   # <= 0: the default
    assert binding.remap_host(acc, x0, len(E), len(S), binding.remap_opts(1e-300))["n_held"] == 0
    r = binding.remap_host(acc, x0, 3, 3)
    assert r["status"] == 0 and r["n_held"] == 0 and not np.any(r["proj"]) and not np.any(r["eigval"]) and np.array_equal(r["start"], x0)
    up = x0.copy(); up[4] = np.pi / 2
    assert binding.remap_host(acc, up, len(E), len(S))["status"] == -3
    bad = acc.copy(); bad[3] = np.nan
    r = binding.remap_host(bad, x0, len(E), len(S))
    assert r["status"] == -2 and r["n_held"] == 0 and not np.any(r["proj"]) and not np.any(r["eigvec"])
    L = binding.lib()
    out = binding.Remap()
    for v in (float("nan"), float("inf"), -float("inf")):
        o = binding.remap_opts(v)
        assert L.alego_remap_host(acc.ctypes.data, x0.ctypes.data, 10, 10, C.byref(o), C.byref(out)) == binding.ERR_ARG, v
    assert L.alego_remap_host(None, x0.ctypes.data, 10, 10, None, C.byref(out)) == binding.ERR_ARG
    assert L.alego_remap_host(acc.ctypes.data, None, 10, 10, None, C.byref(out)) == binding.ERR_ARG
    assert L.alego_remap_host(acc.ctypes.data, x0.ctypes.data, 10, 10, None, None) == binding.ERR_ARG
    assert L.alego_remap_host(acc.ctypes.data, x0.ctypes.data, -1, 10, None, C.byref(out)) == binding.ERR_ARG
    step, mcc, sc = np.zeros(6), C.c_double(), np.ones(6)
    assert L.alego_remap_step_host(None, acc[21:27].ctypes.data, sc.ctypes.data, 1e4, None, step.ctypes.data, C.byref(mcc)) == binding.ERR_ARG
    assert L.alego_remap_step_host(acc.ctypes.data, acc[21:27].ctypes.data, sc.ctypes.data, 1e4, None, None, C.byref(mcc)) == binding.ERR_ARG
    assert L.alego_remap_enable(None, None) == binding.ERR_ARG
