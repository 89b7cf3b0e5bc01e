"""GPU: the collocation Problem with a cost plug-in that has no kernel (opty.direct_collocation, host objective: the host calls
cost / cost_grad, the device solves a sequence of quadratic models over the exact feasible set, d2d_nlp_solve_model).
Checked against the lowered kernel and the committed IPOPT cost where the cost is a known one in disguise, and by a first-order
KKT certificate (and scipy's SLSQP on a short horizon) where no class expresses it."""
import numpy as np
import pytest
from scipy.optimize import lsq_linear, minimize

import d2d.opty_utils as d2ou
import d2d.multiopty_utils as d2mou
import d2d.optyplan_scenarios as d2oscen
import multi_opt_planner as mop
import opty.direct_collocation as dc
import single_opt_planner as sop

pytestmark = pytest.mark.gpu
G = 9.81
IPOPT_EXP14 = 5.02972817          # tests/golden/planner_goldens.npz exp14_cost_airvel12 (the committed IPOPT run)


class Wrapped:
    """A plug-in that is no subclass of anything in d2d: it delegates to another one."""

    def __init__(self, inner):
        self.inner = inner

    def cost(self, free, _p):
        return self.inner.cost(free, _p)

    def cost_grad(self, free, _p):
        return self.inner.cost_grad(free, _p)


class Smooth:
    """CostAirVel(12) + kq sum phi^4 / N + ks sum (v_i - v_{i-1})^2: no class of d2d expresses it."""

    def __init__(self, kq=20., ks=0.002):
        self.kq, self.ks, self.air = kq, ks, d2ou.CostAirVel(12.)

    def cost(self, free, _p):
        return (self.air.cost(free, _p) + self.kq * np.sum(free[_p._slice_phi] ** 4) / _p.num_nodes
                + self.ks * np.sum(np.diff(free[_p._slice_v]) ** 2))

    def cost_grad(self, free, _p):
        g = self.air.cost_grad(free, _p)
        g[_p._slice_phi] += 4 * self.kq * free[_p._slice_phi] ** 3 / _p.num_nodes
        dv = np.diff(free[_p._slice_v])
        gv = np.zeros(_p.num_nodes)
        gv[1:] += 2 * self.ks * dv; gv[:-1] -= 2 * self.ks * dv
        g[_p._slice_v] += gv
        return g


def _jac(W, h, N):
    """Collocation residuals (i = 1..N-1) and end conditions of one aircraft W (5, N): Jacobian rows over its 5N node values
    (component-major, as W.reshape(-1))."""
    x, y, psi, phi, v = W
    rows = []
    I = lambda c, i: c * N + i                                                     # noqa: E731
    for i in range(1, N):
        r0 = np.zeros(5 * N); r0[I(0, i)] = 1 / h; r0[I(0, i - 1)] = -1 / h; r0[I(2, i)] = v[i] * np.sin(psi[i]); r0[I(4, i)] = -np.cos(psi[i])
        r1 = np.zeros(5 * N); r1[I(1, i)] = 1 / h; r1[I(1, i - 1)] = -1 / h; r1[I(2, i)] = -v[i] * np.cos(psi[i]); r1[I(4, i)] = -np.sin(psi[i])
        r2 = np.zeros(5 * N); r2[I(2, i)] = 1 / h; r2[I(2, i - 1)] = -1 / h
        r2[I(3, i)] = -G / v[i] / np.cos(phi[i]) ** 2; r2[I(4, i)] = G * np.tan(phi[i]) / v[i] ** 2
        rows += [r0, r1, r2]
    for i in (0, N - 1):
        for c in range(3):
            r = np.zeros(5 * N); r[I(c, i)] = 1.0
            rows.append(r)
    return np.array(rows)


def _residual(W, h, wind):
    x, y, psi, phi, v = W
    return np.concatenate([np.diff(x) / h - v[1:] * np.cos(psi[1:]) + wind[0], np.diff(y) / h - v[1:] * np.sin(psi[1:]) + wind[1],
                           np.diff(psi) / h - G / v[1:] * np.tan(phi[1:])])


def _kkt(prob, sol, grad):
    """First-order KKT certificate of a solution of prob: least-squares multipliers of the collocation and end equalities, bound
    duals >= 0 on the active boxes.  -> (stationarity residual inf-norm, |g| inf-norm, largest collocation residual)."""
    n, N, h = prob.n_aircraft, prob.num_nodes, prob.time_step
    idx = dc.free_index(n, N, prob.planner)
    W = sol[idx]
    g = grad(sol)[idx].reshape(n, 5 * N)
    feas = max(np.abs(_residual(W[a], h, prob.wind)).max() for a in range(n))
    blocks, gs = [], []
    for a in range(n):
        J = _jac(W[a], h, N).T                                                      # (5N, m)
        cols, lo = [J], [np.full(J.shape[1], -np.inf)]
        bd = prob.bounds[a]
        for c, key in ((0, 'x'), (1, 'y'), (2, 'psi'), (3, 'phi'), (4, 'v')):
            if key not in bd:
                continue
            for side, b in ((+1, bd[key][0]), (-1, bd[key][1])):
                act = np.nonzero(np.abs(W[a, c] - b) <= 1e-5)[0]
                for i in act:
                    e = np.zeros(5 * N); e[c * N + i] = -side                       # grad f + J^T lam - zL + zU = 0, z >= 0
                    cols.append(e[:, None]); lo.append(np.zeros(1))
        A = np.hstack(cols)
        res = lsq_linear(A, -g[a], bounds=(np.concatenate(lo), np.inf), lsmr_tol='auto', tol=1e-13, max_iter=5000)
        blocks.append(np.abs(A @ res.x + g[a]).max())
        gs.append(np.abs(g[a]).max())
    return max(blocks), max(gs), feas


def _bounds_held(prob, sol):
    idx = dc.free_index(prob.n_aircraft, prob.num_nodes, prob.planner)
    W = sol[idx]
    for a, bd in enumerate(prob.bounds):
        for c, key in ((0, 'x'), (1, 'y'), (2, 'psi'), (3, 'phi'), (4, 'v')):
            if key in bd:
                assert (W[a, c] >= bd[key][0]).all() and (W[a, c] <= bd[key][1]).all(), key


@pytest.mark.parametrize('backend', ['nlp', None])
def test_wrapped_known_cost_reproduces_the_lowered_kernel_and_ipopt(backend):
    class exp14w(d2oscen.exp_14):
        cost = Wrapped(d2ou.CostAirVel(12))
    p = sop.Planner(exp14w, backend=backend)
    assert p.prob.objective == 'host'
    p.run(p.get_initial_guess('tri'))
    info = p.info
    assert info['status'] == 1 and info['status_msg'] == 'converged' and info['outer'] <= 4, info
    assert info['backend_used'] == 'nlp' and info['objective'] == 'host'
    c = d2oscen.exp_14.cost.cost(p.solution, p)
    assert abs(c - IPOPT_EXP14) <= 1e-6 * IPOPT_EXP14 and abs(info['obj_val'] - c) <= 1e-14 * c, (c, info)
    assert np.abs(_residual(np.stack([p.sol_x, p.sol_y, p.sol_psi, p.sol_phi, p.sol_v]), p.time_step, (0., 0.))).max() <= 1e-8
    _bounds_held(p.prob, p.solution)
    q = sop.Planner(d2oscen.exp_14, backend='nlp')
    q.run(q.get_initial_guess('tri'))
    assert q.info['status'] == 1 and q.prob.objective == 'lowered'
    assert np.abs(p.solution - q.solution).max() <= 1e-6, np.abs(p.solution - q.solution).max()


def _smooth_scen(kind):
    class s(d2oscen.exp_14):
        cost = Smooth()
    if kind == 'wind':
        s.wind = d2ou.WindField(w=[-1., 0.5])
    elif kind == 'box':                                                            # a turn-around whose free plan reaches x = 47.8
        s.t1, s.p0, s.p1 = 10., (0., 0., 0., 0., 10.), (0., 30., np.pi, 0., 10.)
        s.x_constraint = (-150., 40.)
    elif kind == 'short':
        s.t1, s.p1 = 4., (-20., -30., 0.5, 0., 12.)
        s.p0 = (-49.98, -58.14, 0.9, 0., 12.)
    return s


@pytest.mark.parametrize('kind', ['plain', 'wind', 'box'])
def test_cost_no_class_expresses_meets_a_kkt_certificate(kind):
    scen = _smooth_scen(kind)
    p = sop.Planner(scen, backend='nlp')
    p.run(p.get_initial_guess('tri'))
    assert p.info['status'] == 1, p.info
    st, gmax, feas = _kkt(p.prob, p.solution, p.prob.obj_grad)
    assert feas <= 1e-8 and st <= 1e-6 * (1 + gmax), (st, gmax, feas, p.info)
    _bounds_held(p.prob, p.solution)
    if kind == 'box':
        assert p.sol_x.max() >= 40. - 1e-5                                        # the box binds


def test_cost_no_class_expresses_is_not_worse_than_slsqp():
    scen = _smooth_scen('short')
    p = sop.Planner(scen, backend='nlp')
    assert p.num_nodes <= 41
    x0 = p.get_initial_guess('tri')
    p.run(x0.copy())
    assert p.info['status'] == 1, p.info
    prob, N, h = p.prob, p.num_nodes, p.time_step
    bd = prob.bounds[0]
    lo = np.full(5 * N, -np.inf); hi = np.full(5 * N, np.inf)
    for c, key in ((0, 'x'), (1, 'y'), (3, 'phi'), (4, 'v')):
        if key in bd:
            lo[c * N:(c + 1) * N], hi[c * N:(c + 1) * N] = bd[key]
    ends = np.array(list(scen.p0[:3]) + list(scen.p1[:3]))

    def eq(x):
        W = x.reshape(5, N)
        return np.concatenate([_residual(W, h, (0., 0.)), W[:3, 0], W[:3, -1]]) - np.concatenate([np.zeros(3 * (N - 1)), ends])
    r = minimize(prob.obj, np.clip(x0, lo, hi), jac=prob.obj_grad, method='SLSQP', bounds=list(zip(lo, hi)),
                 constraints=[{'type': 'eq', 'fun': eq, 'jac': lambda x: _jac(x.reshape(5, N), h, N)}],
                 options={'maxiter': 1000, 'ftol': 1e-12})
    if r.success:
        assert p.info['obj_val'] <= r.fun + 1e-6, (p.info['obj_val'], r.fun)


class Sep:
    """Two wrapped CostInput plug-ins + ksep sum_i exp(-d_i^2 / r^2), d_i the distance of the two aircraft at node i."""

    def __init__(self, ksep, r=10.):
        self.parts = [Wrapped(d2mou.CostInput(vsp=12., kv=5., kphi=1.)), Wrapped(d2mou.CostInput(vsp=12., kv=1., kphi=2.))]
        self.ksep, self.r = ksep, r

    def cost(self, free, _p):
        dx = free[_p._slice_x[0]] - free[_p._slice_x[1]]; dy = free[_p._slice_y[0]] - free[_p._slice_y[1]]
        return sum(c.cost(free, _p) for c in self.parts) + self.ksep * np.sum(np.exp(-(dx * dx + dy * dy) / self.r ** 2))

    def cost_grad(self, free, _p):
        g = sum(c.cost_grad(free, _p) for c in self.parts)
        dx = free[_p._slice_x[0]] - free[_p._slice_x[1]]; dy = free[_p._slice_y[0]] - free[_p._slice_y[1]]
        e = self.ksep * np.exp(-(dx * dx + dy * dy) / self.r ** 2) * -2 / self.r ** 2
        g[_p._slice_x[0]] += e * dx; g[_p._slice_x[1]] -= e * dx
        g[_p._slice_y[0]] += e * dy; g[_p._slice_y[1]] -= e * dy
        return g


def _pair(ksep):
    class pair(mop.exp_5):
        t1, hz = 4.2, 10
        p0s = ((0., 0., 0., 0., 12.), (25., -25., np.pi / 2, 0., 12.))           # crossing paths, both at (25, 0) half-way
        p1s = ((50., 0., 0., 0., 12.), (25., 25., np.pi / 2, 0., 12.))
        cost, obj_scale = Sep(ksep), 1.
        x_constraint, y_constraint = None, None
    return pair


def test_two_aircraft_with_a_separation_penalty():
    p = mop.Planner(_pair(0.05), backend='nlp')
    p.run()
    assert p.info['status'] == [1, 1] and p.info['objective'] == 'host', p.info
    st, gmax, feas = _kkt(p.prob, p.solution, p.prob.obj_grad)
    assert feas <= 1e-8 and st <= 1e-6 * (1 + gmax), (st, gmax, feas, p.info)
    _bounds_held(p.prob, p.solution)
    # the penalty pushes the pair apart at the crossing
    p0 = mop.Planner(_pair(0.0), backend='nlp')
    p0.run()
    assert p0.info['status'] == [1, 1]
    d = lambda q: np.hypot(q.solution[q._slice_x[0]] - q.solution[q._slice_x[1]], q.solution[q._slice_y[0]] - q.solution[q._slice_y[1]]).min()  # noqa: E731
    assert d(p) > d(p0) + 0.1, (d(p), d(p0))
    # separation weight 0: each aircraft's plan is the lowered per-aircraft solve
    class low(_pair(0.0)):
        cost = d2mou.CostInput(vsp=12., kv=6., kphi=3.)
    q = mop.Planner(low, backend='nlp')
    q.run()
    assert q.prob.objective == 'lowered' and (np.array(q.info['status']) == 1).all()
    assert np.abs(p0.solution - q.solution).max() <= 1e-6, np.abs(p0.solution - q.solution).max()


def test_inconsistent_gradient_and_nan_cost_end_cleanly():
    class off(d2oscen.exp_14):
        class cost:
            def cost(free, _p):
                return d2ou.CostAirVel(12).cost(free, _p)

            def cost_grad(free, _p):
                return d2ou.CostAirVel(12).cost_grad(free, _p) + 1.0
    p = sop.Planner(off, backend='nlp')
    p.run()
    assert p.info['status'] == 4 and p.info['status_msg'] == 'stalled', p.info
    assert p.info['outer'] <= 60 and np.isfinite(p.solution).all()

    class nan(d2oscen.exp_14):
        class cost:
            def cost(free, _p):
                return float('nan')

            def cost_grad(free, _p):
                return np.zeros_like(free)
    q = sop.Planner(nan, backend='nlp')
    q.run()
    assert q.info['status'] == 3 and q.info['status_msg'] == 'non-finite', q.info
    # the device is fine afterwards: a regular solve
    class exp14w(d2oscen.exp_14):
        cost = Wrapped(d2ou.CostAirVel(12))
    r = sop.Planner(exp14w, backend='nlp')
    r.run()
    assert r.info['status'] == 1 and abs(r.info['obj_val'] - IPOPT_EXP14) <= 1e-6 * IPOPT_EXP14


def test_model_kernel_refuses_a_non_finite_model():
    import d2dhip
    ctx = d2dhip.default_context()
    N = 21
    row = sop.scen_row((0., 0., 0., 0., 12.), (20., 3., 0., 0., 12.), 0., (0., 0., 0., 0., (), float('nan'), 0., 0, 0), 1.0, (0., 0.),
                       (-0.6, 0.6), (9., 15.))
    W0 = np.stack([np.linspace(0, 20, N), np.linspace(0, 3, N), np.zeros(N), np.zeros(N), np.full(N, 12.)])[None]
    H = np.zeros((1, 15, N)); H[:, [0, 5, 9, 12, 14]] = 1.0
    g = np.zeros((1, 5, N))
    outs = []
    for bad in (None, 'g', 'H'):
        gg, HH = g.copy(), H.copy()
        if bad == 'g':
            gg[0, 4, 7] = np.nan
        if bad == 'H':
            HH[0, 3, 2] = np.inf
        dW = ctx.dev(W0)
        out = ctx.nlp_solve_model(ctx.dev(row[None]), dW, 0.1, ctx.dev(gg), ctx.dev(HH), ctx.dev(W0))
        ctx.sync()
        outs.append((int(out['status'][0].item()), float(out['cost'][0].item()), float(out['feas'][0].item())))
    assert outs[0][0] == 1 and outs[0][2] <= 1e-9 and outs[0][1] >= 0.0, outs          # a feasible projection of W0
    for st, c, f in outs[1:]:
        assert st == 3 and np.isnan(c) and np.isnan(f), outs
