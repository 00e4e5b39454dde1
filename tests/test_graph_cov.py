"""Marginal covariances of the key-pose graph and the loop-edge gate (alego_graph_marginals, alego_graph_check_*, the host twin
alego_graph_covariance_host / alego_graph_check_host; csrc/pg_cov_math.h, kernels_pgcov.hip) against numpy's dense
inverse of Lambda = J^T J built from tests/pose_graph_ref.py, which shares no code with the library.

The bound of every comparison: both sides carry a forward error of order eps * cond(Lambda), so |got - reference| <= eps * cond(Lambda) * s
with cond from numpy on the dense Lambda of the case and s the block's scale: max |Sigma_ii| for a marginal, sqrt(max |Sigma_ii| max |Sigma_jj|)
for a pair block, max |P| for P, d2 itself for d2.  Only cases with eps * cond <= 1e-4 are used.  Every test prints the fraction of the bound
it measured."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pose_graph_ref as R
from alego_amd import binding
from test_pose_graph import CONSTRUCTED, I34, _add_loops, _archived_poses, _constructed_handle, _graph_of, drifted_circle
from util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16
CHI2 = binding.GRAPH_CHI2_6_999
NEW_SYMBOLS = ["alego_graph_marginals", "alego_graph_check_edges", "alego_graph_check_loops", "alego_graph_covariance_host", "alego_graph_check_host"]


# ---- the reference ----------------------------------------------------------------------------------------------------
class Dense:
    """Sigma = inv(J^T J) of a graph at X, dense, with cond(Lambda)"""
    def __init__(self, X, g):
        _, J = g.jacobian(X)
        self.lam = (J.T @ J).toarray()
        self.cond = float(np.linalg.cond(self.lam))
        self.sigma = np.linalg.inv(self.lam)
        self.n = len(X)
        self.rel = EPS * self.cond
        assert self.rel <= 1e-4, f"misconstructed case: eps * cond = {self.rel:.2e}"

    def block(self, i, j):
        return self.sigma[6 * i:6 * i + 6, 6 * j:6 * j + 6]

    def marginals(self):
        return np.array([self.block(k, k) for k in range(self.n)])

    def scale(self, i, j):
        return float(np.sqrt(np.abs(self.block(i, i)).max() * np.abs(self.block(j, j)).max()))

    def check(self, X, frm, to, meas, var):
        """(e, P, d2) of the candidate frm -> to by the dense formula"""
        c = R.Graph([frm], [to], [meas], [np.ones(6)])
        e, A, B = c.linearize(X)
        e, A, B = e[0], A[0], B[0]
        Sij = self.block(frm, to)
        P = A @ self.block(frm, frm) @ A.T + B @ self.block(to, to) @ B.T + A @ Sij @ B.T + B @ Sij.T @ A.T + np.diag(var)
        return e, P, float(e @ np.linalg.solve(P, e))


def _frac(got, want, rel, scale):
    return float(np.abs(got - want).max() / (rel * scale))


def _pairs(n):
    return sorted({(0, n - 1), (n - 1, 0), (min(1, n - 1), 0), (n // 2, n // 3)})


# name -> (poses, loops): N = 1, 2, 3; 150 poses with 0 / 1 / 8 loop edges and CONSTRUCTED's layouts (from > to, from < to, a duplicate, nested, crossing); 400 poses
CPU_CASES = {
    "n1": (1, 1.0, ()), "n2": CONSTRUCTED["circle2"][:3], "n3": CONSTRUCTED["circle3"][:3],
    "c150_0": (150, 1.0, ()), "c150_1": CONSTRUCTED["circle150"][:3], "c150_8": CONSTRUCTED["max_loops"][:3],
    "nested": CONSTRUCTED["two_loops_nested"][:3], "crossing_duplicate": CONSTRUCTED["crossing_and_duplicate"][:3], "neighbours": CONSTRUCTED["neighbours"][:3],
    "c400": CONSTRUCTED["circle400"][:3],
}


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    n, drift, loops = CPU_CASES[name]
    X0, g, _ = drifted_circle(n, drift, loops=loops, loop_var=0.1)
    return X0, g, Dense(X0, g)


def _twin(X, g, pairs=()):
    return binding.graph_covariance_host(X, g.frm, g.to, g.meas, g.var, pairs)


def _compare_cov(tag, name, marg, pair, pairs, D):
    want = D.marginals()
    fm = max(_frac(marg[k], want[k], D.rel, np.abs(want[k]).max()) for k in range(D.n))
    fp = max([_frac(pair[p], D.block(i, j), D.rel, D.scale(i, j)) for p, (i, j) in enumerate(pairs)] + [0.0])
    print(f"{tag} {name}: cond {D.cond:.2e} eps*cond {D.rel:.2e}; |{tag} - dense| as a fraction of the bound: marginals {fm:.4f}, pairs {fp:.4f}")
    assert fm <= 1.0 and fp <= 1.0, (name, fm, fp)
    return max(fm, fp)


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_symbols():
    import re
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(binding.lib(), s) and s in binding.EXPORTS, s
    assert CHI2 == float(re.search(r"#define ALEGO_GRAPH_CHI2_6_999 (\S+)", hdr).group(1))
    from scipy.stats import chi2
    assert abs(chi2.ppf(0.999, 6) - CHI2) < 1e-9
    assert C.sizeof(binding.GraphCheck) == 8 + 8 * 43 and C.sizeof(binding.GraphCovResult) == 16


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_host_twin_against_dense_inverse(name):
    X, g, D = cpu_case(name)
    pairs = _pairs(D.n)
    marg, pair = _twin(X, g, pairs)
    _compare_cov("twin", name, marg, pair, pairs, D)


def test_chain_covariance_against_propagation():
    """A reference that inverts nothing: on a chain without loop edges, linearised where its errors are zero, Sigma_00 is the prior's variances
    and Sigma_kk = Ad(h^-1) Sigma_{k-1,k-1} Ad(h^-1)^T + Q_k with h the measured step"""
    X0, _, _ = drifted_circle(150, 1.0, loops=())
    g = R.Graph(*R.chain_graph(X0))
    D = Dense(X0, g)
    marg, _ = _twin(X0, g)
    S = np.diag(g.var[0])
    worst = 0.0
    for k in range(150):
        if k:
            h = g.meas[k]
            Rt = h[:, :3].T
            Ad = np.zeros((6, 6))
            Ad[:3, :3] = Rt; Ad[3:, 3:] = Rt; Ad[3:, :3] = -Rt @ R.hat(h[:, 3])
            S = Ad @ S @ Ad.T + np.diag(g.var[k])
        worst = max(worst, _frac(marg[k], S, D.rel, np.abs(S).max()))
    print(f"propagated chain, 150 poses: cond {D.cond:.2e}; |twin - propagation| as a fraction of the bound: {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_marginals_structure(name):
    """Symmetric TO THE LAST BIT: S_kk, W_k^T W_k and so Sigma_kk are computed on the upper triangle and mirrored (pg_cov_math.h), so both
    halves come from the same operations in the same order.  Positive definite.  Adding a loop edge lowers every marginal."""
    X, g, D = cpu_case(name)
    marg, _ = _twin(X, g)
    for k in range(D.n):
        assert np.array_equal(marg[k], marg[k].T), (name, k)
        assert np.linalg.eigvalsh(marg[k]).min() > 0, (name, k)
    n = D.n
    if len(g.to) == n:
        return
    chain = R.Graph(g.frm[:-1], g.to[:-1], g.meas[:-1], g.var[:-1])   # the same graph without its last loop edge
    before, _ = _twin(X, chain)
    Db = Dense(X, chain)
    low = min(np.linalg.eigvalsh(before[k] - marg[k]).min() / (Db.rel * np.abs(before[k]).max()) for k in range(n))
    print(f"structure {name}: smallest eigenvalue of Sigma_before - Sigma_after as a fraction of the bound: {low:.4f}")
    assert low >= -1.0, (name, low)


HONEST = np.array([2e-3, 2e-3, 2e-3, 1e-2, 1e-2, 1e-2]) ** 2 + np.array([0, 0, 1e-3, 0, 0, 2e-3]) ** 2   # the generator's own noise: sigma^2 + bias^2
DISPLACE = np.array([0, 0, 0.5, 8.0, -5.0, 0])


@functools.lru_cache(maxsize=None)
def gate_case(seed):
    """drifted_circle(150, 1.0, loops = ()) with honest odometry variances; candidates: the true 149 -> 2 measurement, the same displaced by
    0.5 rad of yaw and (8, -5) m, and the true measurement attached to node 60"""
    X0, g, Xt = drifted_circle(150, 1.0, seed=seed, loops=())
    g = R.Graph(g.frm, g.to, g.meas, np.tile(HONEST, (150, 1)))
    true = R.between(Xt[149], Xt[2])
    cands = [("true", 149, 2, true), ("displaced", 149, 2, R.compose(true, R.exp_se3(DISPLACE))), ("wrong_node", 149, 60, true)]
    return X0, g, Dense(X0, g), cands


GATE_DECIDED = [(1, "true"), (2, "true")] + [(s, k) for s in (0, 1, 2) for k in ("displaced", "wrong_node")]   # seed 0's true loop (d2 20.2) lies in the band


def test_check_host_against_dense_formula():
    var = np.full(6, 0.01)
    worst = 0.0
    for seed in (0, 1, 2):
        X, g, D, cands = gate_case(seed)
        got = binding.graph_check_host(X, g.frm, g.to, g.meas, g.var, [c[1] for c in cands], [c[2] for c in cands], [c[3] for c in cands], [var] * len(cands))
        for (kind, i, j, meas), o in zip(cands, got):
            e, P, d2 = D.check(X, i, j, meas, var)
            fd, fP, fe = abs(o["d2"] - d2) / (D.rel * d2), _frac(o["cov"], P, D.rel, np.abs(P).max()), np.abs(o["error"] - e).max()
            worst = max(worst, fd, fP)
            print(f"gate seed {seed} {kind}: d2 twin {o['d2']:.4f} dense {d2:.4f} (eps*cond {D.rel:.2e}); fraction of the bound: d2 {fd:.4f}, P {fP:.4f}; |error diff| {fe:.1e}")
            assert o["status"] == 1 and np.array_equal(o["cov"], o["cov"].T)
            assert fd <= 1.0 and fP <= 1.0 and fe <= 1e-12 * max(1.0, np.abs(e).max()), (seed, kind)
            if (seed, kind) in GATE_DECIDED:
                assert not 0.8 * CHI2 <= d2 <= 1.25 * CHI2, f"misconstructed: seed {seed} {kind} has d2 {d2} inside the band"
                assert (o["d2"] <= CHI2) == (kind == "true"), (seed, kind, o["d2"])
    print(f"gate: largest fraction of the bound {worst:.4f}")


def test_host_misuse():
    L = binding.lib()
    X0, g, _ = drifted_circle(4, 1.0, loops=((3, 0),))
    X = np.ascontiguousarray(X0.reshape(4, 12))
    edges = lambda **kw: binding.graph_edges(**{**dict(frm=g.frm, to=g.to, between=g.meas, variance=g.var), **kw})
    e, n = edges(), len(g.to)
    marg, pair, pr = np.zeros((4, 36)), np.zeros((1, 36)), np.array([[0, 3]], np.int32)
    cov = lambda X_, np_, e_, ne, pr_, npr, m, p: L.alego_graph_covariance_host(X_, np_, e_, ne, pr_, npr, m, p)
    assert cov(X.ctypes.data, 4, e, n, pr.ctypes.data, 1, marg.ctypes.data, pair.ctypes.data) == 0
    assert cov(X.ctypes.data, 4, e, n, None, 0, None, None) == 0                         # n_pairs = 0, every output NULL
    assert cov(None, 4, e, n, None, 0, marg.ctypes.data, None) == binding.ERR_ARG
    assert cov(X.ctypes.data, 0, e, n, None, 0, marg.ctypes.data, None) == binding.ERR_ARG   # n = 0
    assert cov(X.ctypes.data, 4, None, n, None, 0, marg.ctypes.data, None) == binding.ERR_ARG
    assert cov(X.ctypes.data, 4, e, 3, None, 0, marg.ctypes.data, None) == binding.ERR_ARG   # fewer edges than the chain
    assert cov(X.ctypes.data, 4, e, n, None, 1, marg.ctypes.data, pair.ctypes.data) == binding.ERR_ARG
    for bad in ([[0, 4]], [[-1, 0]]):
        b = np.array(bad, np.int32)
        assert cov(X.ctypes.data, 4, e, n, b.ctypes.data, 1, None, pair.ctypes.data) == binding.ERR_ARG, bad
    v0, vneg, frm_bad, to_bad, same = g.var.copy(), g.var.copy(), g.frm.copy(), g.to.copy(), g.frm.copy()
    v0[2, 1] = 0; vneg[4, 0] = -1; frm_bad[4] = 4; to_bad[4] = -1; same[4] = g.to[4]
    chain_bad = g.frm.copy(); chain_bad[2] = 0
    for kw in (dict(variance=v0), dict(variance=vneg), dict(frm=frm_bad), dict(to=to_bad), dict(frm=same), dict(frm=chain_bad)):
        assert cov(X.ctypes.data, 4, edges(**kw), n, None, 0, marg.ctypes.data, None) == binding.ERR_ARG, kw
    Xn = X.copy(); Xn[1, 3] = np.nan
    assert cov(Xn.ctypes.data, 4, e, n, None, 0, marg.ctypes.data, None) == binding.ERR_ARG
    out = (binding.GraphCheck * 2)()
    ok = dict(frm=[3], to=[1], between=[I34], variance=[np.ones(6)])
    chk = lambda X_, e_, c_, nc, o: L.alego_graph_check_host(X_, 4, e_, n, c_, nc, o)
    assert chk(X.ctypes.data, e, binding.graph_edges(**ok), 1, out) == 0 and out[0].status == 1
    assert chk(X.ctypes.data, e, None, 0, None) == 0                                     # n = 0
    assert chk(X.ctypes.data, e, None, 1, out) == binding.ERR_ARG
    assert chk(X.ctypes.data, e, binding.graph_edges(**ok), 1, None) == binding.ERR_ARG
    assert chk(None, e, binding.graph_edges(**ok), 1, out) == binding.ERR_ARG
    nanb = I34.copy(); nanb[0, 0] = np.inf
    for kw in (dict(frm=[4]), dict(frm=[-1]), dict(to=[4]), dict(frm=[1]), dict(variance=[np.array([1, 1, 1, 0, 1, 1.0])]), dict(variance=[-np.ones(6)]),
               dict(variance=[np.full(6, np.inf)]), dict(between=[nanb])):
        assert chk(X.ctypes.data, e, binding.graph_edges(**{**ok, **kw}), 1, out) == binding.ERR_ARG, kw


# ---- the header alone, under AddressSanitizer + UBSan -------------------------------------------------------------------
def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float64).reshape(-1))


def _case_text(X, g, pairs, cands):
    """one case of tests/pg_cov_math/pg_cov_math_check.cpp"""
    lines = [f"{len(X)} {len(g.to)} {len(pairs)} {len(cands)}", _hex(X)]
    lines += [f"{int(f)} {int(t)} {_hex(m)} {_hex(v)}" for f, t, m, v in zip(g.frm, g.to, g.meas, g.var)]
    lines += [f"{i} {j}" for i, j in pairs]
    lines += [f"{int(f)} {int(t)} {_hex(m)} {_hex(v)}" for f, t, m, v in cands]
    return "\n".join(lines) + "\n"


def test_header_under_sanitizers(tmp_path):
    """csrc/pg_cov_math.h compiled for the host with -fsanitize=address,undefined as a program of its own, over the cases of the tests above;
    before them the program holds every function of csrc/pg_chain.h against its plain statement, bit for bit ("pg_chain ok <checks>" on stderr)"""
    exe = str(tmp_path / "pg_cov_math_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # the sanitizers' runtimes are part of the program: nothing has to be preloaded
           "-I" + os.path.join(ROOT, "a-lego-loam_amd", "csrc"), os.path.join(ROOT, "tests", "pg_cov_math", "pg_cov_math_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    var = np.full(6, 0.01)
    jobs = [(name,) + cpu_case(name) + (_pairs(cpu_case(name)[2].n), []) for name in sorted(CPU_CASES)]
    for seed in (0, 1, 2):
        X, g, D, cands = gate_case(seed)
        jobs.append((f"gate{seed}", X, g, D, [], [(i, j, m, var) for _, i, j, m in cands]))
    path = tmp_path / "cases.txt"
    path.write_text("".join(_case_text(X, g, pairs, cands) for _, X, g, _, pairs, cands in jobs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"pg_cov_math ok {len(jobs)}" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    done = [ln for ln in r.stderr.splitlines() if ln.startswith("pg_chain ok ")]
    assert len(done) == 1 and int(done[0].split()[2]) > 0, r.stderr[-3000:]
    print(done[0])
    rows = r.stdout.strip().split("\n")
    assert len(rows) == len(jobs) + 1
    for (name, X, g, D, pairs, cands), row in zip(jobs, rows):
        v = np.array([float.fromhex(x) for x in row.split()])
        n = D.n
        marg, v = v[:n * 36].reshape(n, 6, 6), v[n * 36:]
        pair, v = v[:len(pairs) * 36].reshape(-1, 6, 6), v[len(pairs) * 36:]
        _compare_cov("sanitized header", name, marg, pair, pairs, D)
        for c, (i, j, m, cv) in enumerate(cands):
            st, d2, P = v[c * 44], v[c * 44 + 1], v[c * 44 + 8:c * 44 + 44].reshape(6, 6)
            _, Pw, d2w = D.check(X, i, j, m, cv)
            assert st == 1 and abs(d2 - d2w) <= D.rel * d2w and _frac(P, Pw, D.rel, np.abs(Pw).max()) <= 1.0, (name, c, d2, d2w)


# ---- GPU --------------------------------------------------------------------------------------------------------------
VAR_C = np.full(6, 0.01)
EMPTY = np.zeros((0, 4), np.float32)


def _sixty_four_loops():
    rng = np.random.default_rng(64)
    loops = [(-1, 2)]
    while len(loops) < binding.GRAPH_MAX_LOOPS:
        a, b = (int(v) for v in rng.choice(150, 2, replace=False))
        loops.append((a, b))
    X0, g, _ = drifted_circle(150, 1.0, loops=tuple(loops), loop_var=0.1)
    g.var[150:] = 10.0 ** rng.uniform(-4, np.log10(0.4), (len(loops), 1))
    return X0, R.Graph(g.frm, g.to, g.meas, g.var)


def _device_graphs():
    """N = 1, 2, 3, then 255 / 256 / 257 poses (pgc_blocks' tile of 256 nodes and its neighbours; pgc_correct's tiles of 32 nodes end inside them),
    then 150 poses with 0, 1, 8 and 64 loop edges"""
    out = [drifted_circle(1, 1.0, loops=())[:2], drifted_circle(2, 100.0, loops=((1, 0),))[:2], drifted_circle(3, 80.0, loops=((2, 0),))[:2]]
    out += [drifted_circle(n, 1.0, loops=((-1, 2),))[:2] for n in (255, 256, 257)]
    out += [drifted_circle(150, 1.0, loops=())[:2], drifted_circle(150, 1.0, loops=((-1, 2),))[:2], drifted_circle(150, 1.0, loops=CONSTRUCTED["max_loops"][2])[:2]]
    out.append(_sixty_four_loops())
    return out


def _candidates(s, X):
    """(slot, from, to, measurement) for slot s: node 0 and node N - 1 in both directions, two on the same node pair; 64 for slot 7"""
    n = len(X)
    if n < 2:
        return []
    rng = np.random.default_rng(100 + s)
    near = lambda i, j: R.compose(R.between(X[i], X[j]), R.exp_se3(rng.normal(size=6) * np.array([0.02, 0.02, 0.02, 0.3, 0.3, 0.3])))
    if s == 7:
        pairs = [(n - 1, 0), (0, n - 1)] + [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(62)]
    else:
        pairs = [(0, n - 1), (n - 1, 0), (n - 1, 0), (n // 2, 0)][:4 if n > 2 else 3]
    return [(s, i, j, near(i, j)) for i, j in pairs]


@pytest.fixture(scope="module")
def device():
    graphs = _device_graphs()
    h = _constructed_handle(graphs, binding.GRAPH_MAX_LOOPS, 260)
    for s, (X0, g) in enumerate(graphs):
        _add_loops(h, s, g, len(X0))
    X = [R.from_pose6(_archived_poses(h, s)) for s in range(len(graphs))]
    cands = [c for s in range(len(graphs)) for c in _candidates(s, X[s])]
    dense = [Dense(X[s], g) for s, (_, g) in enumerate(graphs)]
    yield dict(h=h, graphs=graphs, X=X, cands=cands, dense=dense)
    h.close()


def _check_call(h, cands):
    return h.graph_check_edges([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], [c[3] for c in cands], [VAR_C] * len(cands))


@pytest.mark.gpu
def test_device_against_dense_inverse_and_twin(device):
    h, graphs, X, cands, dense = (device[k] for k in ("h", "graphs", "X", "cands", "dense"))
    slots = list(range(len(graphs)))
    res, cov = h.graph_marginals(slots)
    got = _check_call(h, cands)
    worst = worst_twin = 0.0
    for s, (X0, g) in enumerate(graphs):
        D, n = dense[s], len(X0)
        assert (res[s]["status"], res[s]["n_poses"], res[s]["n_loops"]) == (1, n, len(g.to) - n), res[s]
        want = D.marginals()
        twin, _ = _twin(X[s], g)
        f = max(_frac(cov[s, k], want[k], D.rel, np.abs(want[k]).max()) for k in range(n))
        ft = max(np.abs(cov[s, k] - twin[k]).max() / np.abs(want[k]).max() for k in range(n))
        for k in range(n):
            assert np.array_equal(cov[s, k], cov[s, k].T), (s, k)
        assert not cov[s, n:].any()
        mine = [(c, o) for c, o in zip(cands, got) if c[0] == s]
        assert len(mine) == (0 if n < 2 else 64 if s == 7 else 3 if n == 2 else 4)
        th = binding.graph_check_host(X[s], g.frm, g.to, g.meas, g.var, [c[1] for c, _ in mine], [c[2] for c, _ in mine], [c[3] for c, _ in mine], [VAR_C] * len(mine)) if mine else []
        fd = fP = fdt = 0.0
        for (c, o), t in zip(mine, th):
            e, P, d2 = D.check(X[s], c[1], c[2], c[3], VAR_C)
            assert o["status"] == 1 and np.array_equal(o["cov"], o["cov"].T), (s, c[1], c[2])
            assert np.abs(o["error"] - e).max() <= 1e-12 * max(1.0, np.abs(e).max())
            fd, fP = max(fd, abs(o["d2"] - d2) / (D.rel * d2)), max(fP, _frac(o["cov"], P, D.rel, np.abs(P).max()))
            fdt = max(fdt, abs(o["d2"] - t["d2"]) / d2)
        print(f"device slot {s}: {n} poses {len(g.to) - n} loops {len(mine)} candidates, eps*cond {D.rel:.2e}; fraction of the bound: marginals {f:.4f} d2 {fd:.4f} P {fP:.4f}; "
              f"device - twin, relative: marginals {ft:.2e} d2 {fdt:.2e}")
        assert f <= 1.0 and fd <= 1.0 and fP <= 1.0, (s, f, fd, fP)
        worst, worst_twin = max(worst, f, fd, fP), max(worst_twin, ft, fdt)
    print(f"device: largest fraction of the bound {worst:.4f}; largest relative device - twin difference {worst_twin:.2e}")


def _same_checks(tag, a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["status"] == y["status"], (tag, i)
        for k in ("d2", "error", "cov"):
            assert_bit_equal(np.asarray(x[k]), np.asarray(y[k]), f"{tag} candidate {i}: {k}")


@pytest.mark.gpu
def test_independence_of_company_order_and_chunking(device):
    h, graphs, cands = device["h"], device["graphs"], device["cands"]
    slots = list(range(len(graphs)))
    res, cov = h.graph_marginals(slots)
    got = _check_call(h, cands)
    rres, rcov = h.graph_marginals(slots[::-1])
    assert rres[::-1] == res
    assert_bit_equal(rcov[::-1], cov, "reversed: cov36")
    _same_checks("reversed", _check_call(h, cands[::-1])[::-1], got)
    for s in slots:
        r1, c1 = h.graph_marginals([s], cap=cov.shape[1])
        assert r1[0] == res[s]
        assert_bit_equal(c1[0], cov[s], f"slot {s} alone: cov36")
        idx = [i for i, c in enumerate(cands) if c[0] == s]
        if idx:
            _same_checks(f"slot {s} alone", _check_call(h, [cands[i] for i in idx]), [got[i] for i in idx])
    _same_checks("one candidate alone", _check_call(h, cands[-1:]), got[-1:])
    h.set_option("ALEGO_PG_BUDGET", 3 << 20)
    try:
        sres, scov = h.graph_marginals(slots)
        sgot = _check_call(h, cands)
    finally:
        h.set_option("ALEGO_PG_BUDGET", 1 << 30)
    assert sres == res
    assert_bit_equal(scov, cov, "chunked: cov36")
    _same_checks("chunked", sgot, got)


@pytest.mark.gpu
def test_nothing_of_a_slot_moves():
    graphs = [drifted_circle(3, 80.0, loops=((2, 0),))[:2], drifted_circle(150, 1.0, loops=((-1, 2), (-30, 20)))[:2]]
    A, B = (_constructed_handle(graphs, 4, 160) for _ in range(2))
    try:
        for h in (A, B):
            for s, (X0, g) in enumerate(graphs):
                _add_loops(h, s, g, len(X0))
        cands = [c for s in (0, 1) for c in _candidates(s, graphs[s][0])]
        probe = lambda: (A.graph_marginals([1, 0]), _check_call(A, cands))
        first = probe()
        state = lambda h: ([h.graph_status(s) for s in (0, 1)], [_archived_poses(h, s) for s in (0, 1)], [h.graph_get_edges(k, slot=s) for s in (0, 1) for k in (0, 1)])
        sa, sb = state(A), state(B)
        assert sa[0] == sb[0] and sa[0][1][3] == 0
        for x, y in zip(sa[1], sb[1]):
            assert_bit_equal(x, y, "archived poses after the new calls")
        for x, y in zip(sa[2], sb[2]):
            for k in x:
                assert_bit_equal(x[k], y[k], f"edges after the new calls: {k}")
        for rnd in range(2):
            ra, rb = A.graph_optimize([0, 1], max_iters=50, step_tol=1e-10), B.graph_optimize([0, 1], max_iters=50, step_tol=1e-10)
            assert ra == rb and ra[1]["status"] == 2, (ra, rb)
            for s in (0, 1):
                assert_bit_equal(A.graph_get_estimate(slot=s), B.graph_get_estimate(slot=s), f"round {rnd} slot {s}: estimate")
                assert_bit_equal(_archived_poses(A, s), _archived_poses(B, s), f"round {rnd} slot {s}: archived poses")
                assert A.graph_status(s) == B.graph_status(s)
            again = probe()   # between the two optimise calls, and after them: the same answers as before (the archive did not move)
            assert again[0][0] == first[0][0]
            assert_bit_equal(again[0][1], first[0][1], "marginals repeated")
            _same_checks("repeated", again[1], first[1])
    finally:
        A.close(); B.close()


@pytest.mark.gpu
def test_lap_loops_under_the_default_variances():
    """The lap (560 scans, loop search, the reference's default odometry variances): d2 of every accepted loop is finite and within the bound of the
    dense formula on the recorded graph.  No threshold is asserted: the printed values are the noise caveat of DESIGN.md section 20 as a number."""
    import test_loop_search as T
    from test_pose_graph import STEPS, _replay
    p = T._params(False)
    starts = [T.START(0), T.START(37), T.START(64)]
    h = _replay(p, starts, STEPS, True)
    try:
        slots = list(range(len(starts)))
        found = h.loop_search(slots)
        assert any(f["status"] == 2 for f in found), [f["status"] for f in found]
        before = [h.graph_status(s) for s in slots]
        got = h.graph_check_loops(slots, found)
        assert [h.graph_status(s) for s in slots] == before
        for s in slots:
            if found[s]["status"] != 2:
                assert got[s]["status"] == 0 and got[s]["d2"] == 0.0
                continue
            X = R.from_pose6(_archived_poses(h, s))
            D = Dense(X, _graph_of(h, s))
            var = np.full(6, found[s]["noise_variance"])
            e, P, d2 = D.check(X, found[s]["latest_id"], found[s]["closest_id"], found[s]["between"], var)
            fd = abs(got[s]["d2"] - d2) / (D.rel * d2)
            print(f"lap slot {s}: {len(X)} poses, loop {found[s]['latest_id']} -> {found[s]['closest_id']} fitness {found[s]['fitness']:.4f}: d2 device {got[s]['d2']:.3f} "
                  f"dense {d2:.3f} (chi2_6(0.999) = {CHI2:.3f}; |e| {np.abs(e).max():.2e}; eps*cond {D.rel:.2e}; fraction of the bound {fd:.4f})")
            assert got[s]["status"] == 1 and np.isfinite(got[s]["d2"]) and fd <= 1.0, (s, got[s]["d2"], d2)
    finally:
        h.close()


@pytest.mark.gpu
def test_misuse_on_a_handle():
    from alego_amd import synth
    p = synth.default_params(16, 1800)
    err = lambda code: pytest.raises(binding.AlegoError, match=rf"\({code}\)")
    h = binding.Handle(p, n_slots=2)
    try:
        h.map_enable(16, 64)
        for call in (lambda: h.graph_marginals([0], cap=4), lambda: h.graph_check_edges([0], [1], [0], [I34], [VAR_C]), lambda: h.graph_check_loops([0], [])):
            with err(binding.ERR_ARG):
                call()                                          # graph off
    finally:
        h.close()
    h = binding.Handle(p, n_slots=2)
    try:
        h.loc_enable([(np.zeros(6, np.float32), EMPTY, EMPTY, EMPTY)], 0.0)
        with err(binding.ERR_ARG):
            h.graph_marginals([0], cap=4)                       # a localising handle
        with err(binding.ERR_ARG):
            h.graph_check_edges([0], [1], [0], [I34], [VAR_C])
    finally:
        h.close()
    X0, g, _ = drifted_circle(4, 1.0, loops=())
    h = _constructed_handle([(X0, g), (X0[:0], g)], binding.GRAPH_MAX_LOOPS, 8)
    try:
        with err(binding.ERR_ARG):
            h.graph_marginals([0, 1, 0], cap=4)                 # a slot listed twice
        with err(binding.ERR_ARG):
            h.graph_marginals([0], cap=0)                       # cap = 0
        for slot in (-1, 2):
            with err(binding.ERR_ARG):
                h.graph_marginals([slot], cap=4)
            with err(binding.ERR_ARG):
                h.graph_check_edges([slot], [1], [0], [I34], [VAR_C])
        nanb = I34.copy(); nanb[1, 1] = np.nan
        for frm, to, b, var in ((0, 4, I34, VAR_C), (4, 0, I34, VAR_C), (-1, 2, I34, VAR_C), (2, 2, I34, VAR_C), (0, 2, nanb, VAR_C), (0, 2, I34, VAR_C * 0), (0, 2, I34, -VAR_C),
                                (0, 2, I34, VAR_C * np.inf)):
            with err(binding.ERR_ARG):
                h.graph_check_edges([0], [frm], [to], [b], [var])
        with err(binding.ERR_ARG):
            h.graph_check_edges([1], [1], [0], [I34], [VAR_C])  # slot 1 has no frames
        n = binding.GRAPH_MAX_LOOPS
        ok = h.graph_check_edges([0] * n, [3] * n, [0] * n, [I34] * n, [VAR_C] * n)
        assert [o["status"] for o in ok] == [1] * n
        with err(binding.ERR_CAPACITY):
            h.graph_check_edges([0] * (n + 1), [3] * (n + 1), [0] * (n + 1), [I34] * (n + 1), [VAR_C] * (n + 1))   # 65 candidates for one slot
        res, cov = h.graph_marginals([1, 0], cap=2)             # no key frame; a cap below the archive's length keeps a prefix
        assert (res[0]["status"], res[0]["n_poses"]) == (0, 0) and not cov[0].any()
        assert (res[1]["status"], res[1]["n_poses"]) == (1, 4) and cov.shape[1] == 2 and np.linalg.eigvalsh(cov[1, 1]).min() > 0
        assert h.graph_marginals([], cap=4)[0] == [] and h.graph_check_edges([], [], [], [], []) == []   # n = 0
        assert h.graph_status(0) == (4, 0, 0, 0)
    finally:
        h.close()


@pytest.mark.gpu
def test_replay_gate_agrees_with_the_binding():
    """examples/replay N --loop-search EVERY --gate CHI2: a "gate:" line per found loop with the d2 of alego_graph_check_loops, and only the accepted
    edges are added (so the later checks of the run are judged against a graph that holds the earlier ones)"""
    from alego_amd import synth
    from test_loop_search import _scan
    n, every = 440, 20
    exe = os.path.join(ROOT, "examples", "replay")
    out = subprocess.run([exe, str(n), "--loop-search", str(every), "--gate", repr(CHI2)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("gate:")]
    assert len(got) == len([ln for ln in out.stdout.splitlines() if ln.startswith("loop:")])
    p = synth.default_params(16, 1800)
    h = binding.Handle(p)
    try:
        h.map_enable(4096, 1 << 24)
        h.graph_enable(16)
        want = []
        for k in range(n):
            h.scan_process(_scan(p, k), stages=7, stamp=0.1 * k)
            if (k + 1) % every == 0:
                r = h.loop_search([0])
                if r[0]["status"] == 2:
                    c = h.graph_check_loops([0], r)[0]
                    ok = c["status"] == 1 and c["d2"] <= CHI2
                    want.append(f"gate: scan {k} slot 0 d2 {c['d2']:.9g} accepted {int(ok)}")
                    if ok:
                        h.graph_add_loops([0], r)
        print("\n".join(got))
        assert want and got == want, (got, want)
        assert h.graph_status(0)[1] == sum(ln.endswith("accepted 1") for ln in want)
    finally:
        h.close()
