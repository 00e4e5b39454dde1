"""numpy restatement of the solution remapping of LaserMapping's registration (csrc/remap_math.h, lm_solve_remap) and its
constructed cases, shared by tests/test_remap_math.py (host twins) and tests/test_remap_gpu.py (the kernel).  Shares no code with the library:
the projector comes from numpy.linalg.eigh and the explicitly inverted M of regcov_ref, the trust-region loop is tests/lm_control.py's logic
written out once more with the projection in it (lm_control.py itself is left alone)."""
import numpy as np

import regcov_ref as ref

EIG_MIN = 100.0
DELTA = np.array([0.15, 0.08, -0.05, 0.01, -0.008, 0.015])


def projector(acc, p, n_edge, n_plane, eig_min=EIG_MIN):
    """the record of 28 scalars at the start p: status, n_held, eigval, eigvec, proj (parameter space), and the tangent map M"""
    p = np.asarray(p, np.float64)
    out = dict(status=0, n_held=0, start=p.copy(), eigval=np.zeros(6), eigvec=np.zeros((6, 6)), proj=np.zeros((6, 6)), M=np.eye(6))
    if n_edge + n_plane <= 6:
        return out
    if not np.isfinite(p).all():
        return dict(out, status=-2)
    if abs(np.cos(p[4])) < 1e-6:
        return dict(out, status=-3)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = acc[:21]
    H = H + np.triu(H, 1).T
    M = ref.tangent_map(p)
    N = np.linalg.inv(M)
    info = N.T @ H @ N
    info = 0.5 * (info + info.T)
    if not (np.isfinite(acc).all() and np.isfinite(info).all()):
        return dict(out, status=-2)
    lam, V = np.linalg.eigh(info)
    kept = ~(lam < eig_min)
    held = int((~kept).sum())
    Pt = V[:, kept] @ V[:, kept].T
    P = np.eye(6) if held == 0 else (np.zeros((6, 6)) if held == 6 else N @ Pt @ M)
    return dict(out, status=1, n_held=held, eigval=lam, eigvec=V, proj=P, M=M)


def _tri(H21):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = H21
    return H + np.triu(H, 1).T


def step(H21, g, scale, radius, proj=None):
    """one step of the solver at given normal equations: (valid, step in parameter space, model cost change, the step is exactly zero)"""
    Hs = _tri(H21) * np.outer(scale, scale)
    gs = g * scale
    A = Hs + np.diag(np.clip(np.diag(Hs), 1e-6, 1e32) / radius)
    try:
        Lc = np.linalg.cholesky(A)
        st = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, gs))
    except np.linalg.LinAlgError:
        return False, np.zeros(6), 0.0, False
    if not np.all(np.isfinite(st)):
        return False, np.zeros(6), 0.0, False
    null = False
    if proj is not None:
        st = (proj @ (scale * st)) / scale
        if not np.all(np.isfinite(st)):
            return False, np.zeros(6), 0.0, False
        null = bool(np.all(st == 0.0))
    mcc = -(st @ gs) - 0.5 * (st @ Hs @ st)
    if not (mcc > 0.0) and not null:
        return False, np.zeros(6), 0.0, False
    return True, st * scale, float(mcc), null


def solve(evaluate, x0, max_iter, proj=None):
    """one ceres::Solve as the device runs it, every step projected when proj is given -> (x, dict(iterations, successful, termination, initial_cost, final_cost))"""
    x = np.array(x0, np.float64)
    acc = evaluate(x)
    H21, g, x_cost = acc[:21].copy(), acc[21:27].copy(), float(acc[27])
    info = dict(iterations=0, successful=0, termination=0, initial_cost=x_cost, final_cost=x_cost)
    if not np.isfinite(x_cost):
        return x, dict(info, termination=4)
    scale = 1.0 / (1.0 + np.sqrt(_tri(H21).diagonal()))
    x_norm = float(np.linalg.norm(x))
    gmax = float(np.max(np.abs(x - (x - g))))
    radius, dec, it, num_invalid, step_ok = 1e4, 2.0, 0, 0, True
    while True:
        if it >= max_iter:
            info["termination"] = 0
            break
        if step_ok and gmax <= 1e-10:
            info["termination"] = 1
            break
        if radius <= 1e-32:
            info["termination"] = 5
            break
        it += 1
        ok, dx, mcc, _ = step(H21, g, scale, radius, proj)
        if not ok:
            num_invalid += 1
            if num_invalid >= 5:
                info["termination"] = 4
                break
            radius /= dec; dec *= 2.0; step_ok = False
            continue
        num_invalid = 0
        cand = x + dx
        acc = evaluate(cand)
        cand_cost = float(acc[27]) if np.isfinite(acc[27]) else 1.7976931348623157e308
        if np.linalg.norm(x - cand) <= 1e-8 * (x_norm + 1e-8):
            info["termination"] = 2
            break
        change = x_cost - cand_cost
        if abs(change) <= 1e-6 * x_cost:
            info["termination"] = 3
            break
        rd = change / mcc
        if rd > 1e-3:
            x, x_cost, x_norm = cand, cand_cost, float(np.linalg.norm(cand))
            H21, g = acc[:21].copy(), acc[21:27].copy()
            gmax = float(np.max(np.abs(x - (x - g))))
            step_ok = True
            info["successful"] += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rd - 1.0) ** 3))
            dec = 2.0
        else:
            step_ok = False
            radius /= dec; dec *= 2.0
    info["iterations"], info["final_cost"] = it, x_cost
    return x, info


def frame(x0, E, S, remap, eig_min=EIG_MIN, huber=ref.HUBER, max_iter=10, outers=2):
    """a mapping frame's solver part: `outers` solves over the same rows, the projector (remap) taken once at x0 -> what alego_debug_remap_solve returns"""
    x0 = np.asarray(x0, np.float64)
    out = dict(params_it=np.tile(x0, (2, 1)), costs=np.zeros(4), iterations=np.zeros(2, int), successful=np.zeros(2, int), termination=np.zeros(2, int), rec=None)
    rec = projector(ref.normal_equations(x0, E, S, huber), x0, len(E), len(S), eig_min) if len(E) + len(S) else projector(np.zeros(28), x0, 0, 0, eig_min)
    out["rec"] = rec
    if len(E) + len(S) == 0:
        out["termination"][:] = 4
        return out
    proj = rec["proj"] if (remap and rec["status"] == 1 and rec["n_held"] > 0) else None
    x = x0
    for o in range(outers):
        x, info = solve(lambda q: ref.normal_equations(q, E, S, huber), x, max_iter, proj)
        if o < 2:
            out["params_it"][o] = x
            out["costs"][2 * o:2 * o + 2] = info["initial_cost"], info["final_cost"]
            out["iterations"][o], out["successful"][o], out["termination"][o] = info["iterations"], info["successful"], info["termination"]
    if outers < 2:
        out["params_it"][1] = 0.0
    return out


def held_shift(rec, x_final):
    """M0 (x_final - x0) . v_held for every held direction (the tangent space at the start)"""
    xi = rec["M"] @ (np.asarray(x_final) - rec["start"])
    return np.array([rec["eigvec"][:, k] @ xi for k in range(rec["n_held"])])


# ---- constructed cases: name -> (start, edge rows, plane rows, eig_min, held directions) ---------------------------------------------------
def spurious_corridor(n, off, seed):
    """regcov_ref.corridor() plus n wrong plane rows: normal (1, 0, 0), d = -8 — a wall across the corridor at x = 8 — whose query lies `off` metres past it at the corridor's true pose (the residual is +off there, off + 0.15 at the start)"""
    p, E, S = ref.corridor()
    rng = np.random.default_rng(seed)
    world = np.stack([np.full(n, 8.0 + off), rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 2.0, n)], 1)
    q = ((world - p[:3]) @ ref.rot(p)).astype(np.float32).astype(np.float64)
    extra = np.concatenate([np.tile([1.0, 0.0, 0.0, -8.0], (n, 1)), q], 1)
    return p + DELTA, E, np.concatenate([S, extra]), EIG_MIN, 1


def _cases():
    c = {"spurious_3_0.5": spurious_corridor(3, 0.5, 11), "spurious_8_0.3": spurious_corridor(8, 0.3, 12), "spurious_20_0.08": spurious_corridor(20, 0.08, 13)}
    pt = np.array([3.0, 0.2, -0.1, 0.3, -1.0, 2.5])
    p, E, S = ref.corridor(p=pt)
    c["corridor_tilted"] = (p + DELTA, E, S, EIG_MIN, 1)
    p, E, S = ref.courtyard()
    start = p + np.array([0.1, -0.05, 0.04, 0.01, 0.01, -0.01])
    c["courtyard_100"] = (start, E, S, 100.0, 2)
    c["courtyard_10"] = (start, E, S, 10.0, 0)
    c["courtyard_1e5"] = (start, E, S, 1e5, 6)
    return c


CASES = _cases()
SPURIOUS = ("spurious_3_0.5", "spurious_8_0.3", "spurious_20_0.08")


def check_preconditions(name):
    """numpy alone: the held count, no eigenvalue near eig_min, and for the spurious corridors the plain solver's shift along the held direction"""
    x0, E, S, eig_min, held = CASES[name]
    rec = projector(ref.normal_equations(x0, E, S), x0, len(E), len(S), eig_min)
    assert rec["status"] == 1 and rec["n_held"] == held, (name, rec["n_held"], rec["eigval"])
    assert np.all(np.abs(rec["eigval"] - eig_min) > 1e-3 * eig_min), (name, rec["eigval"])
    if name in SPURIOUS:
        plain = frame(x0, E, S, remap=False)
        moved = held_shift(rec, plain["params_it"][1])
        assert abs(moved[0]) > 0.1, (name, moved)
        return rec, moved
    return rec, None
