"""The terminal states of a fit as the oracle states them (include/d2d.h, "Terminal states of a fit"; no GPU): a fit whose first
evaluation is not finite is refused -- ST_NONFINITE, zero iterations, the start point returned, the cost that evaluation gave -- and
a fit stopped by the trial cap reports ST_MAXITER with exactly max_iter iterations, its last accepted point and the cost there.
tests/test_gpu_fit_terminal.py holds the five kernels to the same statements on the same inputs (tests/fit_terminal_ref.py)."""
import numpy as np
import pytest

import fit_terminal_ref as R
from oracle import fit as F, fit_knot as FK


@pytest.fixture(scope='module')
def k50():
    basis = R.oracle_basis('knot50')
    return basis, FK.KnotBasis(basis), R.scenarios('knot50', R.B_REFUSE)


def _solvers(basis, kb):
    return {
        'lm_solve': lambda row, q0: F.lm_solve(basis, row, q0=q0),
        'lm_solve_gn': lambda row, q0: F.lm_solve(basis, row, q0=q0, so_lambda=0.0),
        'solve_minpack': lambda row, q0: F.solve_minpack(basis, row, q0=q0)[:4],
        'solve_minpack_knot': lambda row, q0: FK.solve_minpack_knot(kb, row, q0=q0)[:4],
    }


@pytest.mark.parametrize('kind', R.KINDS)
def test_oracle_refuses_a_fit_whose_first_evaluation_is_not_finite(k50, kind):
    basis, kb, sc = k50
    row = sc[R.HEALTHY_SRC]
    q0 = F.initial_guess(basis, row)
    assert np.isfinite(q0).all() and np.isfinite(F.cost(basis, row, q0))
    bad = R.make_bad(basis, row, q0, kind)
    c0 = R.start_cost(basis, bad, q0)
    if kind == 'overflow':
        assert np.isfinite(bad).all() and np.isposinf(c0)            # a finite row whose cost overflows
    else:
        assert not np.isfinite(bad).all() and not np.isfinite(c0)
        if kind != 'inf_y0':
            assert np.isnan(c0)                                      # NaN in, NaN out
    for name, solve in _solvers(basis, kb).items():
        with np.errstate(all='ignore'):
            q, c, it, st = solve(bad, q0)
        assert st == F.ST_NONFINITE and it == 0, (name, st, it)
        assert q.tobytes() == q0.tobytes(), name                     # the start point itself, not a round trip through other coordinates
        assert (np.isnan(c) and np.isnan(c0)) or c == c0, (name, c, c0)


def test_overflow_scale_is_the_first_power_of_ten_that_overflows(k50):
    basis, _, sc = k50
    row = sc[R.HEALTHY_SRC]
    q0 = F.initial_guess(basis, row)
    s = R.overflow_scale(basis, row, q0)
    below = row.copy(); below[F.SC_S] = s / 10.0
    assert np.isfinite(s) and np.isfinite(R.start_cost(basis, below, q0))


def test_refusal_batches_differ_in_the_bad_rows_only(k50):
    basis, _, _ = k50
    G0 = R.scenarios('knot50', R.B_REFUSE)
    q = np.array([F.initial_guess(basis, G0[R.HEALTHY_SRC if b in R.BAD_ROWS else b]) for b in range(R.B_REFUSE)])
    G, X = R.refusal_batches('knot50', basis, q)
    healthy = [b for b in range(R.B_REFUSE) if b not in R.BAD_ROWS]
    assert len(healthy) == 20 and np.array_equal(G[healthy], X[healthy]) and np.isfinite(G).all()
    for b, kind in zip(R.BAD_ROWS, R.KINDS):
        assert np.array_equal(G[b], G[R.HEALTHY_SRC])
        assert (G[b] != X[b]).sum() == 1 and not np.isfinite(R.start_cost(basis, X[b], q[b])), kind


@pytest.mark.parametrize('name,mode', R.CASES)
def test_oracle_cap_states_and_its_own_precision_split(name, mode):
    """Under max_iter = 1, 2, 5 the sample fits of every (plan, mode): at least a third stopped by the cap, those with iters == max_iter
    exactly, every other with iters <= max_iter; at 5 at least one converges; the cost never above the start's and equal to F.cost at
    the returned point.  And the comparison the GPU test makes with the kernels, made first inside the oracle: its fp32 split (the
    kernels' precision) against its fp64 statement, status, cost and q within 1e-6 on all but at most one fit."""
    basis = R.oracle_basis(name)
    kb = FK.KnotBasis(basis) if R.PLANS[name][3] == 'knot' else None
    rows, q0 = R.sample_fits(name, mode)
    assert rows.shape == (12, F.SCEN_STRIDE) and q0.shape == (12, 2 * basis.nq)
    for cap in R.CAPS:
        n_cap = n_conv = n_out = 0
        for i in range(12):
            a = R.oracle_solve(name, mode, basis, rows[i], q0[i], cap, True, kb)
            b = R.oracle_solve(name, mode, basis, rows[i], q0[i], cap, False, kb)
            n_out += not R.agree(a, b)
            for q, c, it, st in (a, b):
                assert st in (F.ST_CONVERGED, F.ST_STALLED, F.ST_MAXITER) and it <= cap
                assert it == cap if st == F.ST_MAXITER else True
                assert c <= F.cost(basis, rows[i], q0[i]) * (1 + 1e-12)
                assert abs(c - F.cost(basis, rows[i], q)) <= 1e-10 * c
            n_cap += a[3] == F.ST_MAXITER
            n_conv += a[3] == F.ST_CONVERGED
        assert n_cap >= 4, (cap, n_cap)
        assert n_out <= 1, (cap, n_out)
        if cap == 5:
            assert n_conv >= 1
