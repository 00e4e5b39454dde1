"""The key-pose graph's objective restated in numpy / scipy: Pose3 nodes as 3x4 [R | t], a prior on node 0,
Between factors with diagonal variances in GTSAM's tangent order (rotation first), the full SE(3) Logmap / Expmap, analytic
Jacobians for the update x <- x Expmap(delta), and a sparse Gauss-Newton run to stagnation.  The checker of tests/test_pose_graph.py:
it shares no code with the library."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

SERIES_THETA = 0.1
ODOM_VARIANCE = np.array([1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6])


def hat(w):
    z = np.zeros(w.shape[:-1])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1), np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def rzryrx(roll, pitch, yaw):
    cx, sx, cy, sy, cz, sz = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[cy * cz, -cx * sz + sx * sy * cz, sx * sz + cx * sy * cz],
                     [cy * sz, cx * cz + sx * sy * sz, -sx * cz + cx * sy * sz],
                     [-sy, sx * cy, cx * cy]])


def from_pose6(kp):
    """(n, 6) f32 key poses x y z roll pitch yaw -> (n, 3, 4) Pose3(Rot3::RzRyRx(roll, pitch, yaw), xyz) in f64"""
    kp = np.asarray(kp, np.float32).reshape(-1, 6).astype(np.float64)
    X = np.zeros((kp.shape[0], 3, 4))
    for i, k in enumerate(kp):
        X[i, :, :3] = rzryrx(k[3], k[4], k[5])
        X[i, :, 3] = k[:3]
    return X


def to_pose6(X):
    """f32 x y z, roll = atan2(R21, R22), pitch = atan2(-R20, sqrt(R21^2 + R22^2)), yaw = atan2(R10, R00)"""
    X = np.asarray(X, np.float64).reshape(-1, 3, 4)
    out = np.zeros((X.shape[0], 6), np.float32)
    out[:, :3] = X[:, :, 3]
    out[:, 3] = np.arctan2(X[:, 2, 1], X[:, 2, 2])
    out[:, 4] = np.arctan2(-X[:, 2, 0], np.sqrt(X[:, 2, 1] ** 2 + X[:, 2, 2] ** 2))
    out[:, 5] = np.arctan2(X[:, 1, 0], X[:, 0, 0])
    return out


def between(A, B):
    Rt = np.swapaxes(A[..., :3], -1, -2)
    return np.concatenate([Rt @ B[..., :3], Rt @ (B[..., 3:] - A[..., 3:])], -1)


def compose(A, B):
    return np.concatenate([A[..., :3] @ B[..., :3], A[..., :3] @ B[..., 3:] + A[..., 3:]], -1)


def coef_c(th):
    th = np.asarray(th, np.float64)
    t2 = th * th
    ser = 1 / 12 + t2 * (1 / 720 + t2 * (1 / 30240 + t2 * (1 / 1209600 + t2 / 47900160)))
    big = np.where(th < SERIES_THETA, 1.0, th)
    h = 0.5 * big
    return np.where(th < SERIES_THETA, ser, (1 - h * np.cos(h) / np.sin(h)) / (big * big))


def coef_dc(th):
    th = np.asarray(th, np.float64)
    t2 = th * th
    ser = 1 / 360 + t2 * (1 / 7560 + t2 * (1 / 201600 + t2 / 5987520))
    big = np.where(th < SERIES_THETA, 1.0, th)
    h = 0.5 * big
    sh = np.sin(h)
    ex = (-2 / big ** 3 + 1 / (4 * big * sh * sh) + np.cos(h) / sh / (2 * big * big)) / big
    return np.where(th < SERIES_THETA, ser, ex)


def coef_v(th):
    th = np.asarray(th, np.float64)
    t2 = th * th
    ser = 1 / 6 - t2 * (1 / 120 - t2 * (1 / 5040 - t2 * (1 / 362880 - t2 / 39916800)))
    big = np.where(th < SERIES_THETA, 1.0, th)
    return np.where(th < SERIES_THETA, ser, (big - np.sin(big)) / big ** 3)


def log_se3(T):
    """(..., 3, 4) -> (..., 6) = (omega, u)"""
    R, t = T[..., :3], T[..., 3]
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1)
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = np.linalg.norm(v, axis=-1)
    th = np.arctan2(s, c)
    f = np.where(s > 1e-10, th / np.where(s > 1e-10, s, 1.0), 1.0)
    w = f[..., None] * v
    far = c <= -0.5
    if np.any(far):   # beyond 120 degrees the axis comes from the symmetric part (1 - c) a a^T
        S = 0.5 * (R + np.swapaxes(R, -1, -2)) - c[..., None, None] * np.eye(3)
        d = np.diagonal(S, axis1=-2, axis2=-1)
        k = np.where(d[..., 0] >= d[..., 1], np.where(d[..., 0] >= d[..., 2], 0, 2), np.where(d[..., 1] >= d[..., 2], 1, 2))
        a = np.take_along_axis(S, k[..., None, None], -1)[..., 0]
        a = a / np.linalg.norm(a, axis=-1)[..., None]
        sg = np.where((a * v).sum(-1) < 0, -1.0, 1.0)
        w = np.where(far[..., None], (sg * th)[..., None] * a, w)
    wt = np.cross(w, t)
    u = t - 0.5 * wt + coef_c(th)[..., None] * np.cross(w, wt)
    return np.concatenate([w, u], -1)


def exp_se3(xi):
    """(..., 6) -> (..., 3, 4)"""
    xi = np.asarray(xi, np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    th = np.linalg.norm(w, axis=-1)
    ok = th > 1e-10
    ths = np.where(ok, th, 1.0)
    a = np.where(ok, np.sin(ths) / ths, 1.0)[..., None, None]
    b = np.where(ok, 0.5 * (np.sin(0.5 * ths) / (0.5 * ths)) ** 2, 0.5)[..., None, None]
    cv = coef_v(th)[..., None, None]
    W = hat(w)
    W2 = W @ W
    R = np.eye(3) + a * W + b * W2
    V = np.eye(3) + b * W + cv * W2
    return np.concatenate([R, V @ v[..., None]], -1)


def log_jac(T):
    """xi = Logmap(T), J = d Logmap(T Expmap(d)) / d d at 0, (..., 6, 6)"""
    xi = log_se3(T)
    w, t = xi[..., :3], T[..., 3]
    th = np.linalg.norm(w, axis=-1)
    cc, dc = coef_c(th)[..., None, None], coef_dc(th)[..., None, None]
    W = hat(w)
    I = np.eye(3)
    Ji = I + 0.5 * W + cc * (W @ W)
    wdt = (w * t).sum(-1)[..., None, None]
    wwt = np.cross(w, np.cross(w, t))
    D = 0.5 * hat(t) + cc * (wdt * I + w[..., :, None] * t[..., None, :] - 2 * t[..., :, None] * w[..., None, :]) + dc * wwt[..., :, None] * w[..., None, :]
    J = np.zeros(T.shape[:-2] + (6, 6))
    J[..., :3, :3] = Ji
    J[..., 3:, 3:] = Ji
    J[..., 3:, :3] = D @ Ji
    return xi, J


class Graph:
    """edges: from (n,) with -1 = prior on `to`, to (n,), meas (n, 3, 4), var (n, 6)"""
    def __init__(self, frm, to, meas, var):
        self.frm = np.asarray(frm, np.int64)
        self.to = np.asarray(to, np.int64)
        self.meas = np.asarray(meas, np.float64).reshape(-1, 3, 4)
        self.var = np.asarray(var, np.float64).reshape(-1, 6)
        self.sw = 1 / np.sqrt(self.var)

    def errors(self, X):
        pr = self.frm < 0
        Xf = X[np.where(pr, 0, self.frm)]
        h = between(Xf, X[self.to])
        h[pr] = X[self.to[pr]]
        return between(self.meas, h), h

    def residuals(self, X):
        """whitened (n, 6)"""
        e, _ = self.errors(X)
        return log_se3(e) * self.sw

    def linearize(self, X):
        """whitened residuals (n, 6), d res / d delta_from (n, 6, 6; 0 for a prior), d res / d delta_to (n, 6, 6)"""
        e, h = self.errors(X)
        xi, J = log_jac(e)
        Rt = np.swapaxes(h[..., :3], -1, -2)
        Ad = np.zeros_like(J)            # Ad(h^-1)
        Ad[:, :3, :3] = Rt
        Ad[:, 3:, 3:] = Rt
        Ad[:, 3:, :3] = -Rt @ hat(h[..., 3])
        Jf = -(J @ Ad) * self.sw[:, :, None]
        Jf[self.frm < 0] = 0
        return xi * self.sw, Jf, J * self.sw[:, :, None]

    def cost(self, X):
        return float((self.residuals(X) ** 2).sum())

    def jacobian(self, X):
        r, Jf, Jt = self.linearize(X)
        n, N = len(self.to), len(X)
        rows = (6 * np.arange(n)[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64))
        ct = 6 * self.to[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
        be = self.frm >= 0
        cf = 6 * self.frm[be][:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
        J = sp.csr_matrix((np.concatenate([Jt.ravel(), Jf[be].ravel()]), (np.concatenate([rows.ravel(), rows[be].ravel()]), np.concatenate([ct.ravel(), cf.ravel()]))),
                          shape=(6 * n, 6 * N))
        return r.ravel(), J

    def step(self, X):
        r, J = self.jacobian(X)
        H = (J.T @ J).tocsc()
        d = -spl.spsolve(H, J.T @ r)
        return d.reshape(-1, 6)

    def optimize(self, X0, max_iters=60, stagnation=1e-13):
        """plain Gauss-Newton until the largest step component stops falling (or drops below `stagnation`).
        Returns (X, steps = largest |delta| of every iteration, costs = cost before every iteration + the final one)."""
        X = np.array(X0, np.float64).reshape(-1, 3, 4)
        steps, costs = [], [self.cost(X)]
        for _ in range(max_iters):
            d = self.step(X)
            X = compose(X, exp_se3(d))
            steps.append(float(np.abs(d).max()))
            costs.append(self.cost(X))
            if steps[-1] < stagnation or (len(steps) >= 3 and steps[-1] < 1e-9 and steps[-1] >= 0.5 * steps[-2]):
                break
        return X, steps, costs


def chain_graph(X, var=ODOM_VARIANCE):
    """prior on node 0 at X[0] + the odometry chain between consecutive poses"""
    X = np.asarray(X, np.float64).reshape(-1, 3, 4)
    n = len(X)
    meas = np.concatenate([X[:1], between(X[:-1], X[1:])]) if n > 1 else X[:1].copy()
    return np.arange(-1, n - 1), np.arange(n), meas, np.tile(var, (n, 1))
