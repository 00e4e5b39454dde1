"""-m "not gpu": csrc/reg_cov_math.h — the covariance of LaserMapping's scan-to-map registration and its degeneracy — on the host.

tests/reg_cov_math/reg_cov_math_check.cpp is built here with AddressSanitizer and UBSan as a program of its own (the header must be readable
by a host compiler without the HIP runtime): M against finite differences of pg_math.h's Logmap, the Jacobi decomposition on constructed
matrices, every status and every clamp.

The host twins alego_regcov_normal_host + alego_regcov_host are then compared through the binding with tests/regcov_ref.py (stacked Jacobians,
numpy.linalg.inv of the explicit M, numpy.linalg.eigh) on constructed row sets.  Tolerances: the largest deviation from numpy measured over
CASES — the normal equations and info relative to their largest entry, eigenvalues relative to lambda_max, cov and the variances relative to
cov's largest entry, sigma2 relative to itself — and 16 x that asserted, the margin covering numpy's different summation and rotation order:
    measured   normal equations 1.08e-13   info 1.08e-13   eigenvalues 9.88e-14   cov 2.65e-14   sigma2 2.46e-15
    asserted   (16 x)           1.73e-12        1.73e-12             1.58e-12       4.24e-13        3.94e-14
(J^T r is scaled by sqrt(max |H| 2 cost), the bound Cauchy-Schwarz gives its entries.  The largest figures are those of the case with edge
rows only, and they are not 1e-16: an edge row's gradient is the direction of the millimetre-long offset between the query and its line, formed
from a point ten metres out whose own rounding is 2e-15, so two evaluations of one row already differ by 1e-12 of it.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import regcov_ref as ref
from alego_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["alego_regcov_enable", "alego_regcov_get", "alego_regcov_host", "alego_regcov_normal_host", "alego_debug_regcov"]
TOL = dict(acc=1.73e-12, info=1.73e-12, eigval=1.58e-12, cov=4.24e-13, sigma2=3.94e-14)   # 16 x the measured figures of the header


def test_math_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "reg_cov_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "reg_cov_math", "reg_cov_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "reg_cov_math ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_header_library_and_binding_have_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(binding.lib(), s) and s in binding.EXPORTS, s
    assert C.sizeof(binding.RegCov) == 24 + 8 * 122 and C.sizeof(binding.RegCovOpts) == 8 * 16 + 8


# name -> (p, edge rows, plane rows)
def _cases():
    c = {"courtyard": ref.courtyard(), "corridor": ref.corridor(),
         "courtyard_pitched": ref.courtyard(seed=3, p=np.array([-4.0, 2.0, 1.0, -0.4, 1.2, -3.0])),
         "courtyard_yaw_pi": ref.courtyard(seed=4, p=np.array([0.5, 0.5, 0.0, 0.2, -1.2, 3.1])),
         "edges_only": ref.courtyard(n_edge=90, n_plane=0, seed=5), "planes_only": ref.courtyard(n_edge=0, n_plane=90, seed=6),
         "seven_rows": ref.courtyard(n_edge=3, n_plane=4, seed=7), "six_rows": ref.courtyard(n_edge=3, n_plane=3, seed=8)}
    return c


CASES = _cases()


def test_constructed_rows_are_what_they_claim():
    """numpy alone: both sides of Huber's delta occur; the corridor has exactly one eigenvalue below eig_min, along translation x"""
    for name in ("courtyard", "corridor"):
        p, E, S = CASES[name]
        r, _ = ref.rows_jacobian(p, E, S)
        assert (np.abs(r) > ref.HUBER).sum() >= 10 and (np.abs(r) < ref.HUBER).sum() >= 10, name
    p, E, S = CASES["corridor"]
    rec = ref.record(ref.normal_equations(p, E, S), p, len(E), len(S))
    print("corridor eigenvalues", rec["eigval"], "eigenvector of the smallest", rec["eigvec"][:, 0])
    assert rec["status"] == 1 and rec["n_degenerate"] == 1 and (rec["eigval"] < 100.0).sum() == 1
    assert abs(rec["eigvec"][3, 0]) > 0.99
    p, E, S = CASES["courtyard"]
    rec = ref.record(ref.normal_equations(p, E, S), p, len(E), len(S))
    print("courtyard eigenvalues", rec["eigval"])
    assert rec["status"] == 1 and rec["n_degenerate"] == 0


def deviations(got_acc, got, want_acc, want):
    """the figures of the header for one case"""
    f = dict(acc=0.0, info=0.0, eigval=0.0, cov=0.0, sigma2=0.0)
    hs = np.abs(want_acc[:21]).max()
    # (J^T r against the scale Cauchy-Schwarz gives it, sqrt(max |H| 2 cost): its entries are sums that cancel)
    f["acc"] = max(np.abs(got_acc[:21] - want_acc[:21]).max() / hs, np.abs(got_acc[21:27] - want_acc[21:27]).max() / np.sqrt(hs * 2 * want_acc[27]),
                   abs(got_acc[27] - want_acc[27]) / want_acc[27])
    if want["status"] == 1:
        f["info"] = np.abs(got["info"] - want["info"]).max() / np.abs(want["info"]).max()
        f["eigval"] = np.abs(got["eigval"] - want["eigval"]).max() / want["eigval"][-1]
        cs = np.abs(want["cov"]).max()
        f["cov"] = max(np.abs(got["cov"] - want["cov"]).max(), np.abs(got["variance"] - want["variance"]).max()) / cs
        f["sigma2"] = abs(got["sigma2"] - want["sigma2"]) / want["sigma2"]
    return f


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twins_against_numpy(name):
    p, E, S = CASES[name]
    want_acc = ref.normal_equations(p, E, S)
    want = ref.record(want_acc, p, len(E), len(S))
    got_acc = binding.regcov_normal_host(p, E, S, ref.HUBER)
    got = binding.regcov_host(got_acc, p, len(E), len(S))
    f = deviations(got_acc, got, want_acc, want)
    print(f"{name}: deviation from numpy " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
    assert got["status"] == want["status"] == (0 if name == "six_rows" else 1)
    assert (got["n_edge"], got["n_plane"], got["n_degenerate"], got["frame"]) == (len(E), len(S), want["n_degenerate"], 0)
    for k, v in f.items():
        assert v <= TOL[k], (name, k, v, TOL[k])
    if want["status"] == 1:
        assert got["cost"] == got_acc[27] and np.array_equal(got["cov"], got["cov"].T) and np.array_equal(got["info"], got["info"].T)
        assert np.all(np.diff(got["eigval"]) >= 0)
        # eigenvectors: the same lines where the eigenvalue is isolated (a gap of 1e-6 lambda_max on both sides)
        lam = want["eigval"]
        for k in range(6):
            gap = min([abs(lam[k] - lam[m]) for m in range(6) if m != k])
            if gap > 1e-6 * lam[-1]:
                assert abs(abs(got["eigvec"][:, k] @ want["eigvec"][:, k]) - 1.0) < 1e-9, (name, k)
    else:
        assert not np.any(got["info"]) and not np.any(got["cov"]) and not np.any(got["variance"]) and got["cost"] == 0.0 and got["sigma2"] == 0.0


def test_options_through_the_binding():
    p, E, S = CASES["courtyard"]
    acc = binding.regcov_normal_host(p, E, S, ref.HUBER)
    base = binding.regcov_host(acc, p, len(E), len(S))
    o = binding.regcov_opts(sigma0=0.5, scale=2.0, eig_min=1e9, lambda_rel_floor=1e-3, var_min=[1e-12] * 6, var_max=[10.0] * 6)
    got = binding.regcov_host(acc, p, len(E), len(S), o)
    want = ref.record(acc, p, len(E), len(S), sigma0=0.5, scale=2.0, eig_min=1e9, lambda_rel_floor=1e-3, var_min=np.full(6, 1e-12), var_max=np.full(6, 10.0))
    assert got["n_degenerate"] == 6 and got["sigma2"] == 0.25 and base["sigma2"] < 0.25
    assert np.abs(got["variance"] - want["variance"]).max() <= TOL["cov"] * np.abs(want["cov"]).max()
    # the defaults clamp from below with the graph's default odometry variances, from above with 1
    assert np.all(base["variance"] >= ref.ODOM_VAR) and np.all(base["variance"] <= 1.0)
    lo = binding.regcov_host(acc, p, len(E), len(S), binding.regcov_opts(var_min=[0.5] * 6))
    assert np.array_equal(lo["variance"], np.full(6, 0.5))
    hi = binding.regcov_host(acc, p, len(E), len(S), binding.regcov_opts(var_min=[1e-30] * 6, var_max=[1e-20] * 6))
    assert np.array_equal(hi["variance"], np.full(6, 1e-20))
    # misuse of the host calls
    L = binding.lib()
    out = binding.RegCov()
    bad = binding.regcov_opts(var_min=[2.0] * 6)   # above the default var_max
    assert L.alego_regcov_host(acc.ctypes.data, p.ctypes.data, 10, 10, C.byref(bad), C.byref(out)) == binding.ERR_ARG
    assert L.alego_regcov_host(None, p.ctypes.data, 10, 10, None, C.byref(out)) == binding.ERR_ARG
    assert L.alego_regcov_host(acc.ctypes.data, p.ctypes.data, 10, 10, None, None) == binding.ERR_ARG
    assert L.alego_regcov_normal_host(p.ctypes.data, None, 3, None, 0, 0.1, acc.ctypes.data) == binding.ERR_ARG
