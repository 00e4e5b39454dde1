"""pcl::IterativeClosestPoint as performLoopClosure configures it (src/laserMapping.cpp:670-692), written once more in numpy, from the published
rules and not from oracle/oracle_icp.h or csrc/icp_math.h: the rigid transform of an iteration comes from numpy's SVD (Kabsch with the determinant
correction, what pcl::TransformationEstimationSVD / Eigen::umeyama solve), not from Horn's quaternion eigenvector.  tests/test_icp_scenes.py
compares the oracle's loop_icp, alego_loop_closure_icp and alego_loop_search with it.

The project's declared rules are kept: the nearest neighbour is the brute force's in f32 ((dx dx + dy dy) + dz dz), ties to the lowest index, a NaN
or infinite distance never wins; a pair is kept when (double)d2 <= max_corr_dist^2; fewer than 3 pairs end the run unconverged; the transformation
of an iteration is cast to f32, applied to the cloud in f32 and accumulated in f32.
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
DBL_MAX = np.finfo(np.float64).max
ABS_MSE = 1e-12   # DefaultConvergenceCriteria's mse_threshold_absolute_ (PCL's default; performLoopClosure does not set it)


def nn_f32(tgt, q):
    """(index, f32 d2) of the nearest target of every query; (-1, FLT_MAX) where no distance is below FLT_MAX"""
    tgt, q = np.asarray(tgt, F32)[:, :3], np.asarray(q, F32)[:, :3]
    idx = np.full(len(q), -1, np.int64)
    best = np.full(len(q), FLT_MAX, F32)
    if len(tgt) == 0:
        return idx, best
    for b in range(0, len(q), 128):
        Q = q[b:b + 128]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = tgt[None, :, 0] - Q[:, None, 0]
            dy = tgt[None, :, 1] - Q[:, None, 1]
            dz = tgt[None, :, 2] - Q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        d = np.where(np.isnan(d), np.inf, d)
        a = np.argmin(d, axis=1)          # the first of equal minima: the lowest index
        m = d[np.arange(len(Q)), a]
        ok = m < FLT_MAX
        idx[b:b + 128] = np.where(ok, a, -1)
        best[b:b + 128] = np.where(ok, m, FLT_MAX)
    return idx, best


def kabsch(a, b):
    """the rigid (R, t) minimising sum |R a_i + t - b_i|^2 over proper rotations, f64: H = sum (a - ma)(b - mb)^T = U S V^T,
    R = V diag(1, 1, det(V U^T)) U^T, t = mb - R ma.  Also returns the singular values and the sign."""
    a = np.asarray(a, np.float64).reshape(-1, 3)
    b = np.asarray(b, np.float64).reshape(-1, 3)
    ma, mb = a.mean(axis=0), b.mean(axis=0)
    H = (a - ma).T @ (b - mb)
    U, S, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, mb - R @ ma, S, d


def converge(M, mse, prev_mse, it, max_iters, trans_eps, fitness_eps):
    """pcl::registration::DefaultConvergenceCriteria::hasConverged after iteration `it` (counted from 1) whose transformation_ is the f32 M and whose
    correspondences have the mean squared distance mse.  IterativeClosestPoint::computeTransformation hands it max_iterations_, the translation
    threshold transformation_epsilon_ and the rotation threshold 1 - transformation_epsilon_ (PCL 1.8) and the relative MSE euclidean_fitness_epsilon_;
    the absolute MSE threshold stays at its default 1e-12.  Returns (branch, prev_mse afterwards, quantities): branch is one of "iterations",
    "transform", "abs_mse", "rel_mse", None; quantities = [(name, value, threshold)] of every comparison that was made."""
    if it >= max_iters:
        return "iterations", prev_mse, []
    M = np.asarray(M, F32).astype(np.float64).reshape(4, 4)
    cos_angle = 0.5 * (M[0, 0] + M[1, 1] + M[2, 2] - 1.0)
    tr2 = M[0, 3] * M[0, 3] + M[1, 3] * M[1, 3] + M[2, 3] * M[2, 3]
    q = [("1 - cos(angle)", 1.0 - cos_angle, trans_eps), ("translation^2", tr2, trans_eps)]
    if cos_angle >= 1.0 - trans_eps and tr2 <= trans_eps:
        return "transform", prev_mse, q
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dabs = np.float64(abs(mse - prev_mse))
        q.append(("|mse - prev|", float(dabs), ABS_MSE))
        if dabs < ABS_MSE:
            return "abs_mse", prev_mse, q
        rel = dabs / np.float64(prev_mse)
    q.append(("|mse - prev| / prev", float(rel), fitness_eps))
    if rel < fitness_eps:   # (a NaN, 0 / 0, is not below anything)
        return "rel_mse", prev_mse, q
    return None, mse, q


def transform_f32(M, p):
    """pcl::transformPointCloud in f32 with the kernels' order of operations, per component: ((m0 x + m1 y) + m2 z) + m3"""
    M = np.asarray(M, F32).reshape(4, 4)
    p = np.asarray(p, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1)
    assert out.dtype == F32
    return out


def matmul_f32(A, B):
    """Matrix4f A * B, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in f32"""
    A, B = np.asarray(A, F32).reshape(4, 4), np.asarray(B, F32).reshape(4, 4)
    out = np.zeros((4, 4), F32)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return out


def icp(src, tgt, max_corr_dist=100.0, max_iters=100, trans_eps=1e-6, fitness_eps=1e-6):
    """src (n, 3) and tgt (m, 3) f32 in the world frame, the target in the order in which the search sees it (ties go to the lowest index).
    Returns dict(converged, iterations, n_source, n_target, fitness, T (4, 4) f32, trace); trace has one entry per iteration:
    dict(n kept, mse, branch, quantities (see converge), sv and sign (see kabsch), d2 and keep: the f64 squared distance and the filter's verdict for
    every source point that has a nearest neighbour, in source order); branch "too_few" ends a run with fewer than 3 pairs."""
    src = np.ascontiguousarray(np.asarray(src, F32).reshape(-1, 3))
    tgt = np.ascontiguousarray(np.asarray(tgt, F32).reshape(-1, 3))
    res = dict(converged=0, iterations=0, n_source=len(src), n_target=len(tgt), fitness=DBL_MAX, T=np.eye(4, dtype=F32), trace=[])
    if len(src) == 0 or len(tgt) == 0:
        return res
    max2 = float(max_corr_dist) * float(max_corr_dist)
    cur, Tf, prev_mse, it = src.copy(), np.eye(4, dtype=F32), DBL_MAX, 0
    while True:
        idx, d2 = nn_f32(tgt, cur)
        found = idx >= 0
        d2d = d2.astype(np.float64)
        keep = found & (d2d <= max2)
        n = int(keep.sum())
        step = dict(n=n, mse=None, branch=None, quantities=[], d2=d2d[found], keep=keep[found])
        res["trace"].append(step)
        if n < 3:   # "Not enough correspondences found": converged_ = false
            step["branch"] = "too_few"
            break
        a, b = cur[keep].astype(np.float64), tgt[idx[keep]].astype(np.float64)
        mse = float(d2d[keep].sum() / n)
        R, t, S, d = kabsch(a, b)
        M = np.eye(4, dtype=F32)
        M[:3, :3] = R.astype(F32)
        M[:3, 3] = t.astype(F32)
        cur = transform_f32(M, cur)
        Tf = matmul_f32(M, Tf)
        it += 1
        branch, prev_mse, q = converge(M, mse, prev_mse, it, max_iters, trans_eps, fitness_eps)
        step.update(mse=mse, branch=branch, quantities=q, sv=S, sign=d)
        if branch is not None:
            res["converged"] = 1
            break
    res["iterations"], res["T"] = it, Tf
    # getFitnessScore() without a distance limit: the source under the final transformation against the target
    idx, d2 = nn_f32(tgt, transform_f32(Tf, src))
    ok = idx >= 0
    res["fitness"] = float(d2[ok].astype(np.float64).sum() / ok.sum()) if ok.any() else DBL_MAX
    return res
