"""Inputs and reference statements for the terminal states of the trajectory-fit solvers (include/d2d.h, "Terminal states of a fit"):
a fit that is refused (D2D_ST_NONFINITE) and a fit that is stopped by the trial cap (D2D_ST_MAXITER).  Shared by
tests/test_fit_terminal_cpu.py (the oracle states the contract) and tests/test_gpu_fit_terminal.py (the five kernels keep it).

numpy + the oracle only: nothing here touches the GPU."""
import numpy as np

from oracle import fit as F, fit_knot as FK

# ---- the plans: the smallest shapes that reach each kernel --------------------------------------------------------------------
# name -> (S, K, FitPlan(kernel=...), plan.kernel it must report, modes)
PLANS = {
    'knot50': (6, 50, 'auto', 'knot', ('minpack',)),             # the bench's shape: the instantiation with the segment floor
    'knot23': (6, 23, 'auto', 'knot', ('minpack',)),             # segments of 3 and 4 samples: the generic instantiation
    'fused50': (6, 50, 'fused', 'fused', ('minpack', 'fast')),
    'long65': (6, 65, 'auto', 'long', ('minpack', 'fast')),      # the first K past the one-sample-per-lane kernels
    'split40': (4, 40, 'split', 'split', ('default',)),          # eval + step launch pairs, Gauss-Newton rows
}
CASES = [(name, mode) for name, p in PLANS.items() for mode in p[4]]
CAPS = (1, 2, 5)
OBJ_SCALE = 0.1


def plan_consts(name):
    """S, K, duration, wref of a plan (K = 50: bench._plan_consts(); elsewhere the planner's timing at 10 Hz, as tests/test_gpu_knot_segmin.py)."""
    import bench
    from d2dhip import synth
    S, K = PLANS[name][:2]
    if K == bench.K:
        dur, wref = bench._plan_consts()
    else:
        dur, wref = synth.planner_timing(0, (K - 1) / 10.0, 10)[2], synth.default_wref(OBJ_SCALE, K)
    return S, K, dur, wref


def mode_kw(mode):
    """FitPlan.solve / iterate keywords of a mode."""
    import d2dhip
    return {'mode': d2dhip.MODE_FAST} if mode == 'fast' else {}


def scenarios(name, B, seed=5):
    """B bench-style rows for a plan: the bench's own batch at K = 50, the same generator with the distances scaled to the horizon elsewhere."""
    import bench
    from d2dhip import synth
    S, K, dur, _ = plan_consts(name)
    if K == bench.K:
        return bench.bench_scenarios(4096)[:B].copy()       # (the rows other tests take from the bench's batch)
    return synth.synth_scenarios(B, seed=seed, obj_scale=OBJ_SCALE, K=K, dist_range=(30. * dur / 4.9, 55. * dur / 4.9))


N_CAP = 64


def cap_batch(name):
    """The cap tests' batch: 64 bench-style rows, started from the plan's own 'tri' guess."""
    return scenarios(name, N_CAP)


_STARTS = {}


def sample_fits(name, mode):
    """rows [12][SCEN_STRIDE], q0 [12][2 nq]: the twelve fits of (plan, mode) that are compared with the oracle one by one under
    every cap -- started near a minimum, chosen by the oracle alone (tests/golden/make_fit_terminal_golden.py says how and why)."""
    import os
    if not _STARTS:
        _STARTS.update(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fit_terminal_starts.npz'), allow_pickle=False))
    return _STARTS['%s_%s_rows' % (name, mode)].copy(), _STARTS['%s_%s_q0' % (name, mode)].copy()


# ---- the bad rows -------------------------------------------------------------------------------------------------------------
KINDS = ('nan_x1', 'inf_y0', 'nan_wind', 'overflow')
B_REFUSE = 24
BAD_ROWS = (0, 5, 11, 23)              # one of each kind, in the order of KINDS: first and last row of the batch, two inside
HEALTHY_SRC = 1                        # launch G carries copies of this row in their place


def overflow_scale(basis, row, q):
    """The smallest power of ten for D2D_SC_S at which the oracle's cost of (row, q) is +inf -- a finite row whose cost overflows."""
    for e in range(250, 309):
        r = row.copy()
        r[F.SC_S] = float('1e%d' % e)
        with np.errstate(all='ignore'):
            c = F.cost(basis, r, q)
        if np.isposinf(c):
            assert np.isfinite(r).all()
            return r[F.SC_S]
    raise AssertionError('no finite objective scale makes the cost of this row overflow')


def make_bad(basis, row, q, kind):
    """`row` (an ordinary scenario row, started from q) made bad in one way."""
    r = row.copy()
    if kind == 'nan_x1':
        r[F.SC_X1] = np.nan
    elif kind == 'inf_y0':
        r[F.SC_Y0] = np.inf
    elif kind == 'nan_wind':
        r[F.SC_WX] = np.nan
    elif kind == 'overflow':
        r[F.SC_S] = overflow_scale(basis, row, q)
    else:
        raise ValueError(kind)
    return r


def start_cost(basis, row, q):
    """the oracle's cost at the start point, with numpy's floating-point warnings off (the value is the statement)"""
    with np.errstate(all='ignore'):
        return F.cost(basis, row, q)


def refusal_batches(name, basis, q_healthy):
    """(G, X): the all-healthy batch of B_REFUSE rows -- BAD_ROWS hold copies of row HEALTHY_SRC -- and the same batch with one
    bad row of each kind in those places.  q_healthy [B_REFUSE][2 nq]: the start points of G (the bad rows start from them too)."""
    G = scenarios(name, B_REFUSE)
    for b in BAD_ROWS:
        G[b] = G[HEALTHY_SRC]
    X = G.copy()
    for b, kind in zip(BAD_ROWS, KINDS):
        X[b] = make_bad(basis, G[b], q_healthy[b], kind)
    return G, X


def oracle_basis(name):
    S, K, dur, wref = plan_consts(name)
    return F.FitBasis(S, K, dur, wref)


# ---- the oracle's solvers, by plan and mode ----------------------------------------------------------------------------------
def oracle_solve(name, mode, basis, row, q0, max_iter=200, fp32=True, kb=None):
    """q, cost, iterations, status of the oracle's statement of the solver that (plan, mode) runs: solve_minpack_knot for the knot
    plans, solve_minpack / lm_solve for the default / FAST mode of the q kernels, Gauss-Newton lm_solve for the launch pairs.
    fp32: the kernels' precision split (fp32 Hessian and Cholesky factor; residuals, cost and J^T r in fp64)."""
    dt = {'hess_dtype': np.float32, 'chol_dtype': np.float32} if fp32 else {}
    with np.errstate(all='ignore'):
        if PLANS[name][3] == 'knot':
            return FK.solve_minpack_knot(kb if kb is not None else FK.KnotBasis(basis), row, q0=q0, max_iter=max_iter, **dt)[:4]
        if PLANS[name][3] == 'split':
            return F.lm_solve(basis, row, q0=q0, max_iter=max_iter, so_lambda=0.0, **dt)
        if mode == 'fast':
            return F.lm_solve(basis, row, q0=q0, max_iter=max_iter, **dt)
        return F.solve_minpack(basis, row, q0=q0, max_iter=max_iter, **dt)[:4]


def agree(a, b, tol=1e-6):
    """status, cost and q of two solves (q, cost, iters, status) agree within tol relative (q: of its largest entry)"""
    return bool(a[3] == b[3] and abs(a[1] - b[1]) <= tol * abs(b[1]) and np.abs(a[0] - b[0]).max() <= tol * np.abs(b[0]).max())
