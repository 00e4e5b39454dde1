"""The loop-closure ICP (csrc/icp_math.h, kernels_icp.hip, kernels_loop.hip) against references that share no code and no algorithm with it.

1. test_icp_update_against_svd: csrc/icp_math.h compiled for the host (tests/icp_math/icp_math_check.cpp, AddressSanitizer + UBSan, a program of its
   own) runs ONE icp_update per case on sums that this file forms in f64 from point pairs; the answer is compared with numpy's SVD (icp_ref.kabsch) and
   a restatement of DefaultConvergenceCriteria (icp_ref.converge).  This is the test of the claim that Horn's quaternion step finds the minimiser of
   pcl::TransformationEstimationSVD.
2. Constructed scenes (SCENES): the oracle's loop_icp (-m "not gpu"), alego_loop_closure_icp and alego_loop_search (-m gpu) against icp_ref.icp, the
   whole ICP in numpy.  Targets hold one point per lc_leaf voxel, so VoxelGrid only reorders them (asserted), and the reference takes the target in the
   order the API returns.  The reference's own margins are asserted: every convergence quantity of every iteration is at least 2x away from its
   threshold and no pair other than a constructed one lies within 1e-4 (relative) of max_corr_dist^2, so a difference in the last bits cannot move a
   decision and the integer results must agree exactly.

Bounds.  converged, n_source, n_target, iterations: exact.  |T - T_ref| < 1e-5 (tests/test_loop_search.py::check_result's bound; at least 4 f32 ulp at
16 m); for the cloud 3.6 km from the origin the translation column gets 4 f32 ulp of the largest centroid coordinate instead.  Fitness within
1e-6 * max(1, fitness).  The oracle must stay within a tenth of each before a device is compared.

Measured.  icp_update against the SVD (host): M equals the f32 cast of the SVD's answer bit for bit in every case but two, whose entries next to zero
differ by 9e-17 in R and 3e-16 in t, and the 1 m cloud at (2000, -3000, 50): 2.2e-8 in R, 6.5e-5 in t (a quarter of an ulp of 3000).  The oracle against
icp_ref.icp: T and fitness equal bit for bit on every scene but two: 1.8e-15 in "d2 one nextafter beyond max^2" and, far from the origin, 9.5e-7 in T
and 5e-8 in the fitness.  MI355X, alego_loop_closure_icp and alego_loop_search against icp_ref.icp: the same figures as the
oracle's in T (far from the origin 4.7e-10), fitness equal except far from the origin (1.6e-7); the two device paths agree with each other bit for bit in T on
every scene.
"""
import os
import subprocess

import numpy as np
import pytest

import icp_ref
from alego_amd import binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
F64 = np.float64
DBL_MAX = icp_ref.DBL_MAX
DEFAULTS = dict(icp_max_corr_dist=100.0, icp_max_iters=100, icp_trans_eps=1e-6, icp_fitness_eps=1e-6)
T_BOUND, FIT_BOUND = 1e-5, 1e-6


def _O():
    from oracle import oracle_py
    return oracle_py


def rot(axis, ang):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


# ---- 1. one icp_update against the SVD --------------------------------------------------------------------------------------------
GENERAL = np.array([0.3, -0.5, 0.8])


def sums17(a, b, sum_d2=None):
    """the 17 sums of icp_math.h from point pairs, f64: sum a, sum b, sum a_u b_w (row-major u, w), sum of squared distances, count"""
    a, b = np.asarray(a, F64).reshape(-1, 3), np.asarray(b, F64).reshape(-1, 3)
    T = np.zeros(17)
    T[0:3], T[3:6] = a.sum(axis=0), b.sum(axis=0)
    T[6:15] = (a[:, :, None] * b[:, None, :]).sum(axis=0).reshape(9)
    T[15] = ((a - b) ** 2).sum() if sum_d2 is None else sum_d2
    T[16] = len(a)
    return T


def update_cases():
    """(name, a, b, sum of d2 or None, prev_mse, iter, Tf, params, expected branch or Ellipsis for "whatever the rule says")"""
    rng = np.random.default_rng(1)
    I4 = np.eye(4, dtype=F32)
    P = (100.0, 100, 1e-6, 1e-6)
    out = []
    add = lambda name, a, b, sd2=None, prev=DBL_MAX, it=0, Tf=I4, par=P, want=Ellipsis: out.append((name, np.asarray(a, F64), np.asarray(b, F64), sd2, prev, it, Tf, par, want))
    for ang in (0.0, 1e-7, 1e-3, 1.0, np.pi - 1e-3, np.pi - 1e-6, np.pi):
        for axn, ax in (("z", [0, 0, 1]), ("a general axis", GENERAL)):
            a = rng.uniform(-5, 5, (50, 3))
            add(f"angle {ang!r} about {axn}", a, a @ rot(ax, ang).T + [0.3, -0.2, 0.1] + rng.normal(0, 0.01, (50, 3)))
    a = np.c_[rng.uniform(-5, 5, (40, 2)), np.zeros(40)]
    Rm, tm = rot(GENERAL, 0.3), [0.1, 0.2, -0.3]
    add("planar", a, a @ Rm.T + tm)
    at = a @ rot([1, 2, 0.5], 0.7).T
    add("tilted planar", at, at @ Rm.T + tm)
    add("noisy planar", a + rng.normal(0, 1e-3, a.shape), a @ Rm.T + tm + rng.normal(0, 1e-3, a.shape))
    add("mirrored planar", a, a * [1, -1, 1] + rng.normal(0, 1e-3, a.shape) * [1, 1, 0])
    v = rng.uniform(-1, 1, (60, 3)) * [5, 3, 1]
    add("mirrored volume", v, v * [1, 1, -1] + rng.normal(0, 0.01, v.shape))
    tri = np.array([[0, 0, 0], [2, 0.1, 0], [0.3, 1.5, 0.2]])
    add("3 points", tri, tri @ rot(GENERAL, 0.2).T + [0.5, 0, 0])
    add("2 points", tri[:2], tri[:2] + 0.1, prev=0.25, it=7, want="too_few")
    add("identical clouds", v, v.copy())
    far = rng.uniform(-0.5, 0.5, (80, 3)) + [2000, -3000, 50]
    c = far.mean(axis=0)
    add("1 m cloud at (2000, -3000, 50)", far, (far - c) @ rot(GENERAL, 0.02).T + c + [0.1, -0.05, 0.02] + rng.normal(0, 0.005, far.shape))
    Tf = np.eye(4)
    Tf[:3, :3], Tf[:3, 3] = rot([1, -1, 0.2], 0.4), [1.5, -0.5, 0.25]
    a = rng.uniform(-5, 5, (30, 3))
    big = a @ rot(GENERAL, 0.1).T + [0.3, -0.2, 0.1]      # a step far above the transformation epsilon
    add("previous Tf not the identity", a, big + rng.normal(0, 0.01, a.shape), it=3, prev=0.5, Tf=Tf.astype(F32))
    # the convergence rule, each branch away from its threshold on both sides; the sum of d2 is chosen freely (mse = sum / 30)
    n = 30.0
    add("iterations: icp_max_iters = 1", a, big, par=(100.0, 1, 1e-6, 1e-6), want="iterations")
    add("iterations: 99 -> 100 of 100", a, big, it=99, prev=0.5, want="iterations")
    add("iterations: 98 -> 99 of 100", a, big, it=98, prev=0.5, want=None)
    small = lambda ang, t: a @ rot(GENERAL, ang).T + np.array([t, 0, 0])
    add("transformation epsilon: rotation and translation below", a, small(5e-4, 5e-4), want="transform")
    add("transformation epsilon: translation above", a, small(5e-4, 2e-3), want=None)
    add("transformation epsilon: rotation above", a, small(3e-3, 5e-4), want=None)
    add("absolute MSE: below", a, big, sd2=(1e-3 + 4e-13) * n, prev=1e-3, it=5, want="abs_mse")
    add("absolute MSE: above, relative below", a, big, sd2=(1e-3 + 3e-12) * n, prev=1e-3, it=5, want="rel_mse")
    add("absolute MSE: above, relative above", a, big, sd2=(1e-3 + 3e-12) * n, prev=1e-3, it=5, par=(100.0, 100, 1e-6, 1e-10), want=None)
    add("relative MSE: below", a, big, sd2=1.0000004e-3 * n, prev=1e-3, it=5, want="rel_mse")
    add("relative MSE: above", a, big, sd2=1.000003e-3 * n, prev=1e-3, it=5, want=None)
    add("none: the first iteration, prev_mse = DBL_MAX", a, big, want=None)
    add("prev_mse = 0, mse = 0", a, big, sd2=0.0, prev=0.0, it=5, want="abs_mse")
    add("prev_mse = 0, mse > 0", a, big, sd2=1e-3 * n, prev=0.0, it=5, want=None)
    return out


def build_icp_math_check(tmp_path):
    exe = str(tmp_path / "icp_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "icp_math", "icp_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def test_icp_update_against_svd(tmp_path):
    """Bound on M: an entry may differ from the f32 cast of the SVD's answer by 1 f32 ulp of its magnitude.  Two things need a magnitude other than the
    entry's own.  (a) icp_update sees the pairs only through uncentred f64 sums, by design; each product sum carries a rounding error of a few 2^-53 of
    sum |a||b|, and a perturbation dH of the cross-covariance turns the optimal rotation by about |dH| / (s2 + d s3) (s: singular values, d: the sign of
    the determinant correction): F = 8 * 2^-53 * max_uw sum |a_u||b_w| / (s2 + d s3) is added to every rotation entry, and asserted to stay below half an
    ulp of 1, so it only matters where the entry itself is next to zero.  (b) the translation is the difference mean_tgt - R mean_src: its precision is
    that of the centroids, so its ulp is taken at max(|t_i|, the largest centroid coordinate)."""
    cases = update_cases()
    lines = []
    for name, a, b, sd2, prev, it, Tf, par, want in cases:
        v = list(sums17(a, b, sd2)) + [prev, it] + [float(x) for x in np.asarray(Tf, F32).reshape(-1)] + list(par)
        lines.append(" ".join(float(x).hex() for x in v))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = build_icp_math_check(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and f"icp_math ok {len(cases)}" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    rows = r.stdout.strip().split("\n")[:len(cases)]
    worst = dict(R=0.0, t=0.0, R_far=0.0, t_far=0.0)
    seen = set()
    for (name, a, b, sd2, prev, it, Tf, par, want), row in zip(cases, rows):
        w = row.split()
        M = np.array([float.fromhex(x) for x in w[:16]]).reshape(4, 4)
        Tf_out = np.array([float.fromhex(x) for x in w[16:32]]).reshape(4, 4)
        done, conv, it_out, apply_out = int(w[32]), int(w[33]), int(w[34]), int(w[36])
        prev_out = float.fromhex(w[35])
        if len(a) < 3:   # "Not enough correspondences found": the state stays as it was
            assert (done, conv, it_out, prev_out, apply_out) == (1, 0, it, prev, 0), (name, row)
            assert np.array_equal(M, np.eye(4)) and np.array_equal(Tf_out, np.asarray(Tf, F64)), (name, row)
            seen.add("too_few")
            continue
        R, t, S, d = icp_ref.kabsch(a, b)
        assert S[1] > 1e-3 * S[0] and S[1] + d * S[2] > 1e-3 * S[0], (name, S, d)   # one answer
        F = 8 * 2.0 ** -53 * (np.abs(a)[:, :, None] * np.abs(b)[:, None, :]).sum(axis=0).max() / (S[1] + d * S[2])
        assert F <= 2.0 ** -24, (name, F)
        cen = max(np.abs(a.mean(axis=0)).max(), np.abs(b.mean(axis=0)).max())
        M_ref = np.eye(4, dtype=F32)
        M_ref[:3, :3], M_ref[:3, 3] = R.astype(F32), t.astype(F32)
        eR = np.abs(M[:3, :3] - M_ref[:3, :3].astype(F64))
        et = np.abs(M[:3, 3] - M_ref[:3, 3].astype(F64))
        bR = ulp32(M_ref[:3, :3]) + F
        bt = ulp32(np.maximum(np.abs(M_ref[:3, 3].astype(F64)), cen))
        print(f"{name}: |R - R_svd| {eR.max():.3g} ({(eR / bR).max():.3g} of the bound), |t - t_svd| {et.max():.3g} ({(et / bt).max():.3g} of the bound), "
              f"singular values {S / S[0]}, sign {d:+.0f}")
        assert (eR <= bR).all() and (et <= bt).all(), (name, M, M_ref)
        assert np.array_equal(M[3], [0, 0, 0, 1])
        k = "_far" if cen > 100 else ""
        worst["R" + k], worst["t" + k] = max(worst["R" + k], eR.max()), max(worst["t" + k], et.max())
        if "mirrored" in name:
            assert d == -1.0, name
        # final_transformation_ = transformation_ * final_transformation_, in f32 and in this order
        assert np.array_equal(Tf_out, icp_ref.matmul_f32(M.astype(F32), Tf).astype(F64)), (name, Tf_out)
        if not np.array_equal(np.asarray(Tf, F32), np.eye(4, dtype=F32)):
            assert not np.array_equal(Tf_out, icp_ref.matmul_f32(Tf, M.astype(F32)).astype(F64)), "the case cannot tell M Tf from Tf M"
        # the convergence rule on the reference's M; every quantity it compares is 2x away from its threshold
        mse = sums17(a, b, sd2)[15] / len(a)
        branch, prev_ref, q = icp_ref.converge(M_ref, mse, prev, it + 1, par[1], par[2], par[3])
        if want is Ellipsis and q[1][1] >= 2 * q[1][2]:   # a case about the transform, not about the rule: the translation decides the first branch alone
            q = q[1:]
        for what, val, thr in q:
            assert not (thr / 2 < val < 2 * thr), (name, what, val, thr)
        if want is not Ellipsis:
            assert branch == want, (name, branch, want, q)
        seen.add(branch)
        assert (done, conv, it_out, apply_out) == ((1, 1) if branch else (0, 0)) + (it + 1, 1), (name, row, branch)
        assert prev_out == prev_ref, (name, prev_out, prev_ref)
        if branch is None:
            assert prev_out == mse != prev, name
    assert seen == {"too_few", "iterations", "transform", "abs_mse", "rel_mse", None}, seen
    print("worst |M - f32(M_svd)|:", worst)


# ---- 2. constructed scenes --------------------------------------------------------------------------------------------------------
LEAF = 1.0        # lc_leaf of the nodelet's defaults
NOISE = 0.05
ZERO6 = np.zeros(6, F32)


def _pts(xyz):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return np.ascontiguousarray(np.c_[xyz.astype(F32), np.zeros(len(xyz), F32)], dtype=F32)


def split3(a):
    """(corner, surf, outlier) of one cloud; the corner and outlier clouds stay small (a key frame's corner capacity is the smallest)"""
    k = min(len(a) // 3, 200)
    return a[:k], a[2 * k:], a[k:2 * k]


def world_order(n):
    """world(raw)[j] = raw[world_order(n)[j]] + t"""
    k = min(n // 3, 200)
    return np.concatenate([np.arange(2 * k, n), np.arange(0, k), np.arange(k, 2 * k)])


def world(raw3, pose):
    """the cloud as the ICP sees it: surf, corner, outlier (laserMapping.cpp:794-796), each under the key pose.  The scenes' key poses are translations
    (zero angles: the rotation is the identity exactly), so every coordinate is the single f32 addition raw + t."""
    assert not np.asarray(pose[3:]).any()
    c, s, o = split3(np.asarray(raw3, F32).reshape(-1, 3))
    w = np.concatenate([s, c, o])
    if np.asarray(pose[:3]).any():
        with np.errstate(invalid="ignore"):
            w = w + np.asarray(pose[:3], F32)[None, :]
    assert w.dtype == F32
    return w


def voxel_targets(rng, n, half=(8, 8, 2), jitter=0.1, centre=(0, 0, 0)):
    """n points, each in a voxel of its own: the voxel's middle +- jitter, so neighbours are at least 1 - 2 jitter apart.  half[2] == 0: one layer of
    voxels and every point in the plane z = 0.5."""
    hx, hy, hz = half
    cells = np.array([(i, j, k) for k in (range(-hz, hz) if hz else [0]) for j in range(-hy, hy) for i in range(-hx, hx)], F64)
    pick = np.sort(rng.choice(len(cells), n, replace=False))
    return cells[pick] + 0.5 + rng.uniform(-jitter, jitter, (n, 3)) * [1, 1, 1 if hz else 0] + np.asarray(centre, F64)


def lattice(n):
    """the first n points of a 16 x 16 x . lattice of voxel centres (x fastest): VoxelGrid's order is the index order, tile boundaries of the brute-force
    search (2048 targets) fall between z layers 7 and 8, 15 and 16"""
    i = np.arange(n)
    return np.c_[i % 16 - 7.5, (i // 16) % 16 - 7.5, i // 256 - 7.5]


MOTION = (GENERAL, 0.008, np.array([0.08, -0.05, 0.03]))


def moved(tgt_sel, rng, noise=NOISE, motion=MOTION, about=None):
    """sources whose alignment to tgt_sel is the rigid `motion` (axis, angle, translation) about `about`, plus noise"""
    ax, ang, t = motion
    c = np.zeros(3) if about is None else np.asarray(about, F64)
    return (tgt_sel - c - t) @ rot(ax, ang) + c + rng.normal(0, noise, tgt_sel.shape) if noise else (tgt_sel - c - t) @ rot(ax, ang) + c


TIE_SEEDS = {2047: 60, 2048: 60, 2049: 60, 4097: 60}   # (chosen so that the reference's margins hold: test_oracle_against_numpy_icp asserts them)


def tie_scene(n, seed):
    """150 moved sources of the n-point lattice and sources exactly halfway between target k and target k + 256, one z layer up: k from the layers below
    the tile boundaries at 2048 and 4096 (k + 256 lies in the next tile) and three elsewhere"""
    rng = np.random.default_rng(seed)
    lat = lattice(n)
    lower = np.array([k for k in list(range(1792, 2048, 29)) + list(range(3840, 4096, 31)) + [0, 255, 1500] if k + 256 < n])
    return np.concatenate([moved(lat[rng.choice(n, 150, replace=False)], rng), lat[lower] + [0, 0, 0.5]]), lat, lower


def scenes():
    S = {}

    def add(name, src, tgt, expect, pose_src=ZERO6, pose_tgt=ZERO6, far=False, boundary=None, **par):
        assert name not in S
        S[name] = dict(name=name, src=np.asarray(src, F64).reshape(-1, 3).astype(F32), tgt=np.asarray(tgt, F64).reshape(-1, 3).astype(F32), expect=expect,
                       pose_src=np.asarray(pose_src, F32), pose_tgt=np.asarray(pose_tgt, F32), far=far, boundary=boundary, par=dict(DEFAULTS, **par))

    def basic(seed, n_src, n_tgt=None, half=(8, 8, 2), **kw):
        rng = np.random.default_rng(seed)
        tgt = voxel_targets(rng, n_tgt or max(n_src + 37, 300), half)
        sel = rng.choice(len(tgt), n_src, replace=False)
        return moved(tgt[sel], rng, **kw), tgt

    add("volume", *basic(10, 300), "transform")
    add("plane", *basic(11, 200, half=(10, 10, 0)), "transform")
    for n in (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025):
        add(f"n_src {n}", *basic(100 + n, n, half=(10, 10, 2)), "too_few" if n < 3 else "transform")
    # the distance filter keeps some pairs and drops others: outliers sit 0.9 m above targets of the top layer, where no other target is nearer
    def partial(seed, n_in, n_out=40):
        rng = np.random.default_rng(seed)
        tgt = voxel_targets(rng, 500, (8, 8, 2))
        top = np.flatnonzero(tgt[:, 2] > 1.0)
        ax, ang, t = MOTION
        out = (tgt[rng.choice(top, n_out, replace=False)] + [0, 0, 0.9] - t) @ rot(ax, ang)
        rest = np.setdiff1d(np.arange(len(tgt)), top)
        return np.concatenate([moved(tgt[rng.choice(rest, n_in, replace=False)], rng), out]), tgt
    add("partial filter, 300 inliers", *partial(20, 300), "transform", icp_max_corr_dist=0.5)
    add("partial filter, 3 inliers", *partial(21, 3), "transform", icp_max_corr_dist=0.5)
    add("partial filter, 2 inliers", *partial(22, 2), "too_few", icp_max_corr_dist=0.5)
    # d2 == max^2 exactly and one nextafter beyond: sources coincide with their targets except the last, 0.5 m outside the +x face of the lattice
    # (boundary = its index in the cloud as stored)
    lat = lattice(16 * 16 * 2)
    face = lat[lat[:, 0] == 7.5][21]
    for name, x in (("d2 == max^2", F32(8.0)), ("d2 one nextafter beyond max^2", np.nextafter(F32(8.0), F32(np.inf)))):
        add(name, np.concatenate([lat[5:400:7], [[x, face[1], face[2]]]]), lat, "iterations", icp_max_corr_dist=0.5, icp_max_iters=1, boundary=len(lat[5:400:7]))
    add("icp_max_iters 1", *basic(30, 300), "iterations", icp_max_iters=1)
    add("icp_max_iters 2", *basic(30, 300), "iterations", icp_max_iters=2)
    # small coordinates and no noise: after the second iteration the MSE is rounding noise of about 1e-14 and stops changing
    add("absolute MSE", *basic(31, 100, n_tgt=140, half=(3, 3, 2), noise=0.0), "abs_mse", icp_trans_eps=1e-30, icp_fitness_eps=1e-30)
    add("relative MSE", *basic(32, 300), "rel_mse", icp_trans_eps=1e-30, icp_fitness_eps=1e-2)
    # the brute-force search's tiles: sources halfway between two lattice targets one z layer apart, on both sides of every tile boundary
    for n, seed in TIE_SEEDS.items():
        src, lat, lower = tie_scene(n, seed)
        add(f"n_tgt {n}", src, lat, "transform")
        # run to the end, an alignment can forget how its first ties were broken (with 2047 targets the other rule, the highest index, ends 2e-7 away);
        # after one iteration it cannot: T moves by 0.02 to 0.08
        add(f"n_tgt {n}, one iteration", src, lat, "iterations", icp_max_iters=1)
        S[f"n_tgt {n}"]["ties"] = S[f"n_tgt {n}, one iteration"]["ties"] = (len(src) - len(lower), lower)
    rng = np.random.default_rng(45)
    one = np.array([[0.5, 0.5, 0.5]])
    add("n_tgt 1", np.concatenate([one + [[0.1, 0.05, -0.2], [-0.2, 0.1, 0.1]], one + rng.uniform(1, 3, (38, 3)) * rng.choice([-1, 1], (38, 3))]), one, "too_few", icp_max_corr_dist=0.5)
    src, tgt = basic(50, 200)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 1, 2], [1, 2, np.nan], [np.nan, np.nan, np.nan]])
    add("non-finite source points", np.insert(src, [0, 60, 61, 150, 200], bad, axis=0), tgt, "transform")
    # 3.6 km from the origin: f32 coordinates have a resolution of 2.4e-4 m
    rng = np.random.default_rng(51)
    C = np.array([2000, -3000, 50])
    tgt = voxel_targets(rng, 200, (3, 3, 3), centre=C)
    add("far from the origin", moved(tgt[rng.choice(200, 150, replace=False)], rng, about=C), tgt, "iterations", far=True, icp_max_iters=1)
    src, tgt = basic(52, 100)
    add("empty source", np.zeros((0, 3)), tgt, "empty")
    add("empty target", src, np.zeros((0, 3)), "empty")
    # key poses that are not the identity: both clouds are stored relative to their own key pose
    src, tgt = basic(53, 250)
    ps, pt = np.array([1.0, -2.0, 0.5, 0, 0, 0], F32), np.array([-0.75, 0.25, 1.5, 0, 0, 0], F32)
    add("non-zero key poses", src - ps[:3].astype(F64), tgt - pt[:3].astype(F64), "transform", pose_src=ps, pose_tgt=pt)
    return S


SCENES = scenes()
NAMES = list(SCENES)


def params_of(sc):
    p = synth.default_params(16, 1800)
    p.lc_search_num = 0
    assert p.lc_leaf == LEAF
    for k, v in sc["par"].items():
        setattr(p, k, v)
    return p


def frames_of(sc):
    """[(pose, corner, surf, outlier)]: the newest key frame (source), then the one history frame (target)"""
    return [(sc["pose_src"],) + tuple(_pts(c) for c in split3(sc["src"])), (sc["pose_tgt"],) + tuple(_pts(c) for c in split3(sc["tgt"]))]


def assert_permutation(got, want, tag):
    """the same rows, bit for bit, in any order"""
    g, w = np.ascontiguousarray(got, F32).reshape(-1, 3), np.ascontiguousarray(want, F32).reshape(-1, 3)
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    gs, ws = g[np.lexsort(g.T[::-1])], w[np.lexsort(w.T[::-1])]
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"{tag}: VoxelGrid changed a point of a cloud with one point per voxel"


_REF = {}


def reference(name):
    """(icp_ref's result, the oracle's result, the target in search order) of a scene, computed once.  The target's order is the oracle's VoxelGrid order;
    the GPU test asserts that the device returns the same."""
    if name not in _REF:
        sc = SCENES[name]
        want, tgt = _O().loop_icp(params_of(sc), frames_of(sc))
        wt = world(sc["tgt"], sc["pose_tgt"])
        assert (tgt[:, 3] == 0).all()
        assert_permutation(tgt[:, :3], wt, name)
        par = sc["par"]
        ref = icp_ref.icp(world(sc["src"], sc["pose_src"]), tgt[:, :3], par["icp_max_corr_dist"], par["icp_max_iters"], par["icp_trans_eps"], par["icp_fitness_eps"])
        _REF[name] = (ref, want, tgt)
    return _REF[name]


def t_bound(sc, ref):
    """per entry of T"""
    b = np.full((4, 4), T_BOUND)
    if sc["far"]:   # 4 f32 ulp of the coordinate magnitude at the centroid, for the translation
        b[:3, 3] = 4 * ulp32(np.abs(world(sc["tgt"], sc["pose_tgt"]).astype(F64).mean(axis=0)).max())
    return b


def compare(got, ref, sc, tag, scale=1.0):
    """one implementation's result against icp_ref's: integers exact, T and fitness within scale * the bound; returns the deviations"""
    assert (got["converged"], got["n_source"], got["n_target"], got["iterations"]) == (ref["converged"], ref["n_source"], ref["n_target"], ref["iterations"]), \
        (tag, {k: got[k] for k in ("converged", "n_source", "n_target", "iterations")}, {k: ref[k] for k in ("converged", "n_source", "n_target", "iterations")})
    dT = np.abs(np.asarray(got["T"], F64).reshape(4, 4) - ref["T"].astype(F64))
    assert (dT < scale * t_bound(sc, ref)).all(), (tag, dT.max(), got["T"], ref["T"])
    if ref["fitness"] == DBL_MAX:
        assert got["fitness"] == DBL_MAX, (tag, got["fitness"])
        dF = 0.0
    else:
        dF = abs(got["fitness"] - ref["fitness"])
        assert dF < scale * FIT_BOUND * max(1.0, ref["fitness"]), (tag, got["fitness"], ref["fitness"])
    return dT.max(), dF


def test_scene_list_is_the_issue_list():
    par = lambda k: {SCENES[n]["par"][k] for n in NAMES}
    assert {1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025} <= {len(SCENES[n]["src"]) for n in NAMES}
    assert {1, 2047, 2048, 2049, 4097} <= {len(SCENES[n]["tgt"]) for n in NAMES}
    assert par("icp_max_iters") == {1, 2, 100} and par("icp_max_corr_dist") == {0.5, 100.0}
    assert {SCENES[n]["expect"] for n in NAMES} == {"transform", "iterations", "abs_mse", "rel_mse", "too_few", "empty"}
    for n in NAMES:
        sc = SCENES[n]
        lim = 16.0 if not sc["far"] else 3100.0
        for c in (sc["src"], sc["tgt"]):
            assert len(c) == 0 or np.nanmax(np.abs(np.where(np.isfinite(c), c, 0))) <= lim, n
        if len(sc["tgt"]):   # one point per lc_leaf voxel, in the world frame
            v = np.floor(world(sc["tgt"], sc["pose_tgt"]).astype(F64) / LEAF)
            assert len(np.unique(v, axis=0)) == len(v), n


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_numpy_icp(name):
    """the oracle's loop_icp against icp_ref.icp within a tenth of the bounds, and the reference's own margins"""
    sc = SCENES[name]
    ref, want, tgt = reference(name)
    par, trace = sc["par"], ref["trace"]
    last = trace[-1]["branch"] if trace else "empty"
    print(f"{name}: n_src {ref['n_source']} n_tgt {ref['n_target']} iterations {ref['iterations']} converged {ref['converged']} fitness {ref['fitness']:.6g} "
          f"branches {[s['branch'] for s in trace]} kept {[s['n'] for s in trace]}")
    assert last == sc["expect"], (name, last, sc["expect"])
    max2 = par["icp_max_corr_dist"] ** 2
    for k, step in enumerate(trace):
        for what, val, thr in step["quantities"]:
            assert not (thr / 2 < val < 2 * thr), (name, k, what, val, thr)
        near = np.flatnonzero(np.abs(step["d2"] / max2 - 1.0) < 1e-4)
        if sc["boundary"] is not None and k == 0:
            at = int(np.flatnonzero(world_order(len(sc["src"])) == sc["boundary"])[0])
            assert near.tolist() == [at], (name, near, at)
            assert step["keep"][at] == (step["d2"][at] == max2), name
        else:
            assert len(near) == 0, (name, k, near, step["d2"][near])
        if step["branch"] != "too_few":
            assert step["sv"][1] > 1e-3 * step["sv"][0], (name, k, step["sv"])
    if "partial" in name:
        assert 0 < trace[0]["n"] < ref["n_source"] and trace[0]["n"] == ref["n_source"] - 40, (name, trace[0]["n"])
    if name == "d2 == max^2":
        assert trace[0]["n"] == ref["n_source"]
    if name == "d2 one nextafter beyond max^2":
        assert trace[0]["n"] == ref["n_source"] - 1
    if "ties" in sc:
        # the scene sees the tie rule: with ties to the highest index instead (the reversed target) the reference's T moves by a thousand times the bound
        if par["icp_max_iters"] == 1:
            other = icp_ref.icp(world(sc["src"], sc["pose_src"]), tgt[::-1, :3], par["icp_max_corr_dist"], 1, par["icp_trans_eps"], par["icp_fitness_eps"])
            assert np.abs(other["T"].astype(F64) - ref["T"].astype(F64)).max() > 1000 * T_BOUND, name
        # each halfway source is exactly as far from the lower target as from the upper one, which lies in another tile where the target has one
        first, lower = sc["ties"]
        src_w, t3 = world(sc["src"], sc["pose_src"]), tgt[:, :3]
        assert np.array_equal(t3, lattice(len(t3)).astype(F32)), "VoxelGrid's order of the lattice is its index order"
        mid = src_w[np.argsort(world_order(len(src_w)))][first:]
        idx, d2 = icp_ref.nn_f32(t3, mid)
        assert np.array_equal(idx, lower) and (d2 == 0.25).all(), (name, idx, lower)
        dz = t3[lower + 256] - mid
        assert (((dz * dz).sum(axis=1)) == 0.25).all()
        if len(t3) > 2048:
            assert (lower // 2048 != (lower + 256) // 2048).sum() == {2049: 1, 4097: 10}[len(t3)], name   # (4097: nine into tile 1, one into tile 2)
    if (sc["expect"] in ("transform", "rel_mse") or "icp_max_iters" in name or sc["far"]) and ref["n_source"] >= 63:   # 0.05 m of noise: the fitness is not rounding noise
        assert ref["fitness"] > NOISE ** 2, (name, ref["fitness"])
    dT, dF = compare(want, ref, sc, name, scale=0.1)
    print(f"    oracle vs numpy: |T - T_ref| {dT:.3g}, |fitness - ref| {dF:.3g}")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_results():
    """{name: (alego_loop_closure_icp's result and target, alego_loop_search's result)}: one handle per set of ICP parameters, one slot per scene,
    every slot's archive built with alego_lm_add_keyframe (frame 0 = target, frame 1 = source) and searched in one call"""
    groups = {}
    for n in NAMES:
        groups.setdefault(tuple(sorted(SCENES[n]["par"].items())), []).append(n)
    out = {}
    for names in groups.values():
        p = params_of(SCENES[names[0]])
        h = binding.Handle(p, n_slots=len(names))
        h.map_enable(4, 1 << 13)
        for s, n in enumerate(names):
            fr = frames_of(SCENES[n])
            h.lm_add_keyframe(fr[1][0], *fr[1][1:], slot=s)
            h.lm_add_keyframe(fr[0][0], *fr[0][1:], slot=s)
            assert h.map_status(s)[:2] == (2, 0), n
            h.map_set_stamps(0, np.array([0.0, 100.0]), slot=s)   # the target is old enough (lc_min_time_gap)
        found = h.loop_search(list(range(len(names))))
        for s, n in enumerate(names):
            out[n] = (h.loop_closure_icp(frames_of(SCENES[n])), found[s])
        h.close()
    return out


_WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_against_numpy_icp(device_results, name):
    sc = SCENES[name]
    ref, want, tgt = reference(name)
    (one, one_tgt), found = device_results[name]
    assert np.array_equal(one_tgt.view(np.uint32), tgt.view(np.uint32)), f"{name}: the device's target differs from the oracle's (order included)"
    assert (found["status"], found["latest_id"], found["closest_id"]) == (2 if ref["converged"] and ref["fitness"] <= params_of(sc).lc_fitness_max else 1, 1, 0), (name, found)
    d1 = compare(one, ref, sc, f"{name}: alego_loop_closure_icp")
    d2 = compare(found, ref, sc, f"{name}: alego_loop_search")
    assert (one["converged"], one["iterations"], one["n_source"], one["n_target"]) == (found["converged"], found["iterations"], found["n_source"], found["n_target"]), name
    dd = np.abs(one["T"].astype(F64) - found["T"].astype(F64)).max()
    assert (np.abs(one["T"].astype(F64) - found["T"].astype(F64)) < t_bound(sc, ref)).all(), (name, one["T"], found["T"])
    if ref["fitness"] != DBL_MAX:
        assert abs(one["fitness"] - found["fitness"]) < FIT_BOUND * max(1.0, ref["fitness"]), (name, one["fitness"], found["fitness"])
    k = "far" if sc["far"] else "near"
    w = _WORST.setdefault(k, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], d1[0], d2[0]), max(w[1], d1[1], d2[1]), max(w[2], dd)
    print(f"{name}: |T - T_ref| single attempt {d1[0]:.3g}, search {d2[0]:.3g}, between the two {dd:.3g}; |fitness - ref| {d1[1]:.3g}, {d2[1]:.3g}; "
          f"running maxima (T vs ref, fitness vs ref, T between the paths) {_WORST}")
