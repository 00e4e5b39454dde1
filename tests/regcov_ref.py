"""numpy restatement of the registration covariance (csrc/reg_cov_math.h, lm_regcov) and constructed row sets, shared by
tests/test_reg_cov_math.py (host twins) and tests/test_regcov_gpu.py (the kernel).  Shares no code with the library: the normal equations are
formed from stacked Jacobians, M is written out and inverted by numpy.linalg.inv, the eigen-decomposition is numpy.linalg.eigh."""
import numpy as np

HUBER = 0.1
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6])
DEFAULTS = dict(sigma0=0.02, scale=1.0, eig_min=100.0, lambda_rel_floor=1e-12, var_min=ODOM_VAR, var_max=np.ones(6))


def rot(p):
    """R = Rz(yaw) Ry(pitch) Rx(roll) of p = (x, y, z, roll, pitch, yaw)"""
    sr, cr, sp, cp, sy, cy = np.sin(p[3]), np.cos(p[3]), np.sin(p[4]), np.cos(p[4]), np.sin(p[5]), np.cos(p[5])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def tangent_map(p):
    """M: xi = M dp, right perturbation, rotation first"""
    sr, cr, sp, cp = np.sin(p[3]), np.cos(p[3]), np.sin(p[4]), np.cos(p[4])
    E = np.array([[1.0, 0, -sp], [0, cr, sr * cp], [0, -sr, cr * cp]])
    M = np.zeros((6, 6))
    M[:3, 3:] = E
    M[3:, :3] = rot(p).T
    return M


def _table(p, pts):
    """d (R pt) / d roll, pitch, yaw as the cost functors of the reference write them (the pitch column of y keeps its cr sr cp term)"""
    sr, cr, sp, cp, sy, cy = np.sin(p[3]), np.cos(p[3]), np.sin(p[4]), np.cos(p[4]), np.sin(p[5]), np.cos(p[5])
    X, Y, Z = pts[:, 0], pts[:, 1], pts[:, 2]
    d_dr = np.stack([(cy * sp * cr + sr * sy) * Y + (sy * cr - cy * sr * sp) * Z, (-cy * sr + sy * sp * cr) * Y + (-sr * sy * sp - cy * cr) * Z, cp * cr * Y - cp * sr * Z], 1)
    d_dp = np.stack([-cy * sp * X + cy * cp * sr * Y + cy * cr * cp * Z, -sp * sy * X + sy * cp * sr * Y + cr * sr * cp * Z, -cp * X - sp * sr * Y - sp * cr * Z], 1)
    d_dy = np.stack([-sy * cp * X - (sy * sp * sr + cr * cy) * Y + (cy * sr - sy * cr * sp) * Z, cp * cy * X + (-sy * cr + cy * sp * sr) * Y + (cy * cr * sp + sy * sr) * Z, 0 * X], 1)
    return d_dr, d_dp, d_dy


def rows_jacobian(p, edges, planes):
    """residuals (n,) and Jacobians (n, 6) of edge rows (a, b, pt) (n, 9) and plane rows (normal, d, pt) (m, 7) at p, edges first"""
    p = np.asarray(p, np.float64)
    R, t = rot(p), p[:3]
    edges, planes = np.asarray(edges, np.float64).reshape(-1, 9), np.asarray(planes, np.float64).reshape(-1, 7)
    res, jac = [], []
    if len(edges):
        a, b, pt = edges[:, 0:3], edges[:, 3:6], edges[:, 6:9]
        lp = pt @ R.T + t
        k = np.linalg.norm(a - b, axis=1)
        c = np.cross(lp - a, lp - b)
        m = np.linalg.norm(c, axis=1)
        g = np.cross(c, b - a) / m[:, None]   # d |(lp - a) x (lp - b)| / d lp
        d_dr, d_dp, d_dy = _table(p, pt)
        J = np.concatenate([g, np.stack([(g * d_dr).sum(1), (g * d_dp).sum(1), (g * d_dy).sum(1)], 1)], 1) / k[:, None]
        res.append(m / k); jac.append(J)
    if len(planes):
        n, d, pt = planes[:, 0:3], planes[:, 3], planes[:, 4:7]
        lp = pt @ R.T + t
        d_dr, d_dp, d_dy = _table(p, pt)
        J = np.concatenate([n, np.stack([(n * d_dr).sum(1), (n * d_dp).sum(1), (n * d_dy).sum(1)], 1)], 1)
        res.append((n * lp).sum(1) + d); jac.append(J)
    if not res:
        return np.zeros(0), np.zeros((0, 6))
    return np.concatenate(res), np.concatenate(jac)


def normal_equations(p, edges, planes, huber=HUBER):
    """the 28 scalars: upper triangle of J^T J (Huber-corrected rows), J^T r, 1/2 sum rho"""
    r, J = rows_jacobian(p, edges, planes)
    s, b2 = r * r, huber * huber
    out = s > b2
    ar = np.sqrt(np.where(out, s, 1.0))
    sq = np.where(out, np.sqrt(huber / ar), 1.0)
    rho = np.where(out, 2 * huber * ar - b2, s)
    Jc, rc = J * sq[:, None], r * sq
    H, g = Jc.T @ Jc, Jc.T @ rc
    return np.concatenate([H[np.triu_indices(6)], g, [0.5 * rho.sum()]])


def record(acc, p, n_edge, n_plane, **opts):
    """the record of 28 scalars at p as a dict, by numpy"""
    o = dict(DEFAULTS, **opts)
    rows = n_edge + n_plane
    out = dict(status=0, n_edge=n_edge, n_plane=n_plane, n_degenerate=0, cost=0.0, sigma2=0.0, info=np.zeros((6, 6)), eigval=np.zeros(6), eigvec=np.zeros((6, 6)),
               cov=np.zeros((6, 6)), variance=np.zeros(6))
    if rows <= 6:
        return out
    if abs(np.cos(p[4])) < 1e-6:
        return dict(out, status=-3)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = acc[:21]
    H = H + np.triu(H, 1).T
    Mi = np.linalg.inv(tangent_map(np.asarray(p, np.float64)))
    info = Mi.T @ H @ Mi
    info = 0.5 * (info + info.T)
    if not (np.isfinite(acc).all() and np.isfinite(p).all() and np.isfinite(info).all()):
        return dict(out, status=-2)
    lam, V = np.linalg.eigh(info)
    sigma2 = max(o["sigma0"] ** 2, 2 * acc[27] / (rows - 6))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / np.maximum(lam, o["lambda_rel_floor"] * lam[-1])
        cov = sigma2 * (V * w) @ V.T
    if not (np.isfinite(cov).all() and np.isfinite(sigma2)):
        return dict(out, status=-2)
    var = np.clip(o["scale"] * np.diag(cov), o["var_min"], o["var_max"])
    return dict(out, status=1, n_degenerate=int((lam < o["eig_min"]).sum()), cost=float(acc[27]), sigma2=float(sigma2), info=info, eigval=lam, eigvec=V, cov=cov, variance=var)


# ---- constructed row sets ---------------------------------------------------------------------------------------------
def _to_sensor(p, world):
    """sensor-frame query points (rounded to f32, as the device keeps them) of world points at pose p"""
    return ((world - p[:3]) @ rot(p)).astype(np.float32).astype(np.float64)


def make_rows(p, lines, planes, seed, noise=0.01, outliers=0.1, outlier_size=0.4):
    """lines: (point on the line (3), unit direction (3), n); planes: (point on the plane (3), unit normal (3), two in-plane extents, n).
    Every query lies near its feature: an offset of `noise` (inliers, |r| < Huber's delta) or about outlier_size (the first row of every
    feature and a fraction `outliers` of the others, |r| > delta), so both branches of the loss occur in any set of two rows or more."""
    rng = np.random.default_rng(seed)
    p = np.asarray(p, np.float64)
    E, S = [], []
    for c, d, n in lines:
        c, d = np.asarray(c, float), np.asarray(d, float)
        d = d / np.linalg.norm(d)
        for i in range(n):
            w0 = c + d * rng.uniform(-3, 3)
            off = np.cross(d, rng.normal(size=3))
            off *= (outlier_size * rng.uniform(0.8, 1.5) if (rng.uniform() < outliers or i == 0) else noise * rng.uniform(0.1, 2.0)) / np.linalg.norm(off)
            E.append(np.concatenate([w0 + 0.1 * d, w0 - 0.1 * d, _to_sensor(p, w0 + off)]))
    for c, nrm, ext, n in planes:
        c, nrm = np.asarray(c, float), np.asarray(nrm, float)
        nrm = nrm / np.linalg.norm(nrm)
        u = np.cross(nrm, [0.3, 0.5, 0.8]); u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        for i in range(n):
            w0 = c + u * rng.uniform(-ext, ext) + v * rng.uniform(-ext, ext)
            h = (outlier_size * rng.uniform(0.8, 1.5) if (rng.uniform() < outliers or i == 0) else noise * rng.uniform(0.1, 2.0)) * rng.choice([-1.0, 1.0])
            S.append(np.concatenate([nrm, [-float(nrm @ c)], _to_sensor(p, w0 + h * nrm)]))
    return np.array(E).reshape(-1, 9), np.array(S).reshape(-1, 7)


P_COURTYARD = np.array([1.0, -2.0, 0.5, 0.05, -0.03, 0.7])
P_CORRIDOR = np.array([3.0, 0.2, -0.1, 0.01, -0.015, 0.02])


def courtyard(n_edge=120, n_plane=300, seed=1, p=P_COURTYARD):
    """planes with three independent normals and lines along all three axes around the sensor"""
    ne, npl = max(n_edge // 3, 0), max(n_plane // 3, 0)
    lines = [((6, 4, 0), (0, 0, 1), ne), ((-5, 7, 1), (1, 0, 0), ne), ((4, -6, 2), (0.1, 1, 0), n_edge - 2 * ne)]
    planes = [((0, 0, -1.5), (0, 0, 1), 8, npl), ((9, 0, 1), (1, 0.05, 0), 5, npl), ((0, -8, 1), (0, 1, 0.02), 5, n_plane - 2 * npl)]
    return (p,) + make_rows(p, [l for l in lines if l[2] > 0], [q for q in planes if q[3] > 0], seed)


def corridor(seed=2, p=P_CORRIDOR):
    """a corridor along x: no plane normal has an x component, every line is parallel to x — translation along x is unconstrained"""
    lines = [((0, 1.9, 2.2), (1, 0, 0), 30), ((0, -1.9, 2.2), (1, 0, 0), 30), ((0, 1.9, -1.2), (1, 0, 0), 20)]
    planes = [((3, 2, 0.5), (0, 1, 0), 6, 120), ((3, -2, 0.5), (0, -1, 0), 6, 120), ((3, 0, -1.3), (0, 0, 1), 6, 100), ((3, 0, 2.4), (0, 0.02, -1), 6, 60)]
    return (p,) + make_rows(p, lines, planes, seed)
