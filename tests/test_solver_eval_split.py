"""-m gpu: the solvers' cost-first evaluation against the evaluation of every point in full.

lo_solve_t and lm_solve evaluate a trust-region candidate for its cost alone and the normal equations only at points a further step is
computed from (csrc/solve_rows.h: lm_propose_lazy, lm_control).  ALEGO_SOLVE_FULL_EVAL=1 selects the kernels that evaluate every point in
full with eval_block + accumulate_block, call for call the solver before the split.  Nothing may differ: one handle of each kind runs the
same scans, and after every scan everything the two solvers leave behind is compared bit for bit.
"""
import numpy as np
import pytest

from alego_amd import binding, synth
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

# scal (fe_store.h): SC_LO_NSURF, SC_LO_NCORNER, SC_LO_FLAGS, SC_LO_ITERS, SC_LO_ITERS2
SC_LO = slice(7, 12)
# lm_info (lm_ctx.h): LI_NCC, LI_NSC, LI_SUM0, LI_SUM1 and their neighbours; lm_state: everything up to the timing words of development builds
LI_SOLVE = slice(6, 12)
LD_SOLVE = slice(0, 43)


def _summary(word):
    """(iterations, successful steps, termination) of a packed solver summary"""
    word = int(word)
    return word & 0xFF, (word >> 8) & 0xFF, word >> 16


def _run_pair(p, n_scans, monkeypatch, row_lds=None):
    """One default handle and one ALEGO_SOLVE_FULL_EVAL=1 handle over the same scans; returns the default handle's solver summaries:
    {"lo_surf": [...], "lo_corner": [...], "lm0": [...], "lm1": [...]} of (iterations, successful, termination)."""
    if row_lds is None:
        monkeypatch.delenv("ALEGO_LM_ROW_LDS", raising=False)
    else:
        monkeypatch.setenv("ALEGO_LM_ROW_LDS", row_lds)
    monkeypatch.delenv("ALEGO_SOLVE_FULL_EVAL", raising=False)
    hd = binding.Handle(p)
    monkeypatch.setenv("ALEGO_SOLVE_FULL_EVAL", "1")
    hf = binding.Handle(p)
    monkeypatch.delenv("ALEGO_SOLVE_FULL_EVAL", raising=False)
    seen = {"lo_surf": [], "lo_corner": [], "lm0": [], "lm1": []}
    optimised = 0
    for k in range(n_scans):
        pts = synth.scan(p, k)
        (_, od, md), (_, of, mf) = hd.scan_process(pts, stages=7), hf.scan_process(pts, stages=7)
        tag = f"scan {k}"
        # LaserOdometry: params_ after the surf solve and final, the four costs, t_w_cur_ / r_w_cur_ (lo_state); counts, flags, both summaries
        assert_bit_equal(hd.debug_get("lo_state"), hf.debug_get("lo_state"), f"{tag} LO state (params_, params_ after the surf solve, costs)")
        sd, sf = hd.debug_get("scal"), hf.debug_get("scal")
        assert_bit_equal(sd[SC_LO], sf[SC_LO], f"{tag} LO correspondence counts / flags / solver summaries")
        # LaserMapping: params_ per outer iteration, costs, the poses (lm_state); correspondence counts and summaries (lm_info)
        ld, lf = hd.debug_get("lm_state"), hf.debug_get("lm_state")
        assert_bit_equal(ld[LD_SOLVE], lf[LD_SOLVE], f"{tag} LM state (params_, params_ per outer iteration, costs, poses)")
        gd, gf = hd.debug_get("lm_info"), hf.debug_get("lm_info")
        assert_bit_equal(gd[LI_SOLVE], gf[LI_SOLVE], f"{tag} LM correspondence counts / solver summaries")
        for a, b, name in ((od, of, "odometry"), (md, mf, "map")):
            for key in ("t", "q", "params"):
                assert_bit_equal(a[key], b[key], f"{tag} {name} pose {key}")
        if k > 0:
            seen["lo_surf"].append(_summary(sd[10])); seen["lo_corner"].append(_summary(sd[11]))
        if gd[11]:   # LI_OPTIMIZED: lm_solve ran for this frame
            optimised += 1
            seen["lm0"].append(_summary(gd[8])); seen["lm1"].append(_summary(gd[9]))
    hd.close(); hf.close()
    assert optimised >= 2, f"only {optimised} optimised mapping frames"
    return seen


def _accepted(s):
    return any(succ > 0 for _, succ, _ in s)


def _not_adopted(s):
    """a candidate that was evaluated and not adopted: rejected by the trust region, or the one that ended the solve"""
    return any(it > succ for it, succ, _ in s)


def _rejected(s):
    """a candidate the trust region rejected, after which the solve went on (terminations 2 and 3 spend their last iteration on the
    candidate that ends the solve; invalid steps are not evaluated at all, and none occurs in these streams)"""
    return any(it - succ - (1 if term in (2, 3) else 0) > 0 for it, succ, term in s)


def test_defaults_16x1800(monkeypatch):
    """30 scans at the defaults.  The premise is asserted from the summaries.  Each of the two odometry solves saw adopted candidates and
    candidates the trust region rejected in mid-solve; the odometry ended solves on its iteration limit (the adopted point of the last permitted
    iteration never gets a Jacobian) and on the cost change.  LaserMapping's first solve saw adopted candidates and, in every frame, the
    candidate that ends the solve on the cost change (evaluated, not adopted); its second solve that candidate alone.  No LaserMapping solve of
    these streams rejects a step and goes on (the oracle's summaries of the same scans: iterations = successful + 1, termination 3, in every
    frame), so that path is not asserted here: it is the same lm_control as the odometry's, and tests/solve_rows/solve_rows_check.cpp drives it
    on edge + plane problems with rejected steps on the host."""
    seen = _run_pair(synth.default_params(16, 1800), 30, monkeypatch)
    for name in ("lo_surf", "lo_corner", "lm0"):
        assert _accepted(seen[name]), f"{name}: no accepted step in {seen[name]}"
    for name in ("lo_surf", "lo_corner"):
        assert _rejected(seen[name]), f"{name}: no step rejected in mid-solve in {seen[name]}"
    for name in ("lm0", "lm1"):
        assert _not_adopted(seen[name]), f"{name}: every candidate was adopted in {seen[name]}"
    terms = {t for _, _, t in seen["lo_surf"] + seen["lo_corner"]}
    assert 0 in terms and 3 in terms, f"odometry terminations {terms}: want the iteration limit (0) and the cost change (3)"
    assert {t for _, _, t in seen["lm0"]} == {3}, f"LaserMapping terminations {seen['lm0']}"


@pytest.mark.parametrize("lm_max_iters", [1, 2])
def test_lm_iteration_limit(lm_max_iters, monkeypatch):
    """The solve ends on the iteration limit with an adopted point that was evaluated for its cost only: the next outer iteration has to
    evaluate the normal equations for itself."""
    p = synth.default_params(16, 1800)
    p.lm_max_iters = lm_max_iters
    seen = _run_pair(p, 30, monkeypatch)
    assert any(term == 0 and succ == it == lm_max_iters for it, succ, term in seen["lm0"]), f"no solve ended on the limit with every step accepted: {seen['lm0']}"


def test_lo_one_iteration(monkeypatch):
    p = synth.default_params(16, 1800)
    p.lo_iters_surf = p.lo_iters_corner = 1
    seen = _run_pair(p, 30, monkeypatch)
    assert all(it <= 1 for it, _, _ in seen["lo_surf"] + seen["lo_corner"])


def test_huber_corrector(monkeypatch):
    """huber_delta = 0.01: many rows are outliers of the loss and take the corrector.  That rows do is read off the first solve of scan 1, which
    starts from the same point on the same rows whatever the loss: its initial cost (lo_state[24]) is smaller than with the default delta of
    0.1 exactly when rows lie beyond 0.01 there (rho = 2 delta |r| - delta^2 < r^2 for them, rho = r^2 for the rest)."""
    p = synth.default_params(16, 1800)
    monkeypatch.delenv("ALEGO_SOLVE_FULL_EVAL", raising=False)
    cost0 = {}
    for delta in (p.huber_delta, 0.01):
        p.huber_delta = delta
        h = binding.Handle(p)
        for k in range(2):
            h.scan_process(synth.scan(p, k), stages=7)
        cost0[delta] = float(h.debug_get("lo_state")[24])
        h.close()
    assert 0.0 < cost0[0.01] < cost0[0.1], f"initial cost of scan 1's surf solve {cost0}: no row beyond delta = 0.01"
    _run_pair(p, 30, monkeypatch)


@pytest.mark.parametrize("row_lds", ["0", "20000", "44", "60", "104"])
def test_rows_from_hbm(row_lds, monkeypatch):
    """lm_solve's rows beyond the LDS budget come from `crows`: all of them, and the split inside the lists.  44, 60 and 104 bytes cut where
    the split of the budget (lml_split, csrc/lm_rows.h: 60 B an edge, 44 B a plane, edges first) has its edges: no edge resident and one plane,
    one edge and no plane, one of each.  Those three run 6 scans: mapping frames are scans 1, 3, 5, the first finds no map yet, so 6 is the
    fewest scans with the two optimised frames _run_pair asks for."""
    _run_pair(synth.default_params(16, 1800), 30 if row_lds in ("0", "20000") else 6, monkeypatch, row_lds=row_lds)


def test_lo_rows_not_staged(monkeypatch):
    """Feature counts raised until the handle's row capacity exceeds what lo_solve_t stages in LDS (640 rows): the rows stream from HBM.
    (6 x 6 + 3 x 6) x 16 rings = 864 rows: beyond 640, short of the wide kernel's 1024."""
    p = synth.default_params(16, 1800)
    p.n_flat, p.n_sharp = 6, 3
    assert (p.n_flat + p.n_sharp) * p.n_sectors * p.n_scan > 640 and (p.n_flat + p.n_sharp) * p.n_sectors * p.n_scan <= 1024
    _run_pair(p, 30, monkeypatch)


def test_wide_64x2048(monkeypatch):
    """64 rings: the 256-thread lo_solve_t"""
    p = synth.default_params(64, 2048)
    assert (p.n_flat + p.n_sharp) * p.n_sectors * p.n_scan > 1024
    _run_pair(p, 6, monkeypatch)
