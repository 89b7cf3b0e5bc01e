"""CPU: the collocation Problem accepts objectives that have no kernel (a user's cost plug-in, plain callables) and selects the
host objective; the curvature builder of that path recovers the per-node Hessian blocks from 15 cost_grad calls per aircraft;
the polynomial fit still refuses such a cost, with its reason."""
import numpy as np
import pytest

import d2d.opty_utils as d2ou
import d2d.optyplan_scenarios as d2oscen
import opty.direct_collocation as dc
import single_opt_planner as sop
import multi_opt_planner as mop


class Comfort:
    """A cost plug-in no class of d2d expresses: s sum (v - 12)^2 + s kq sum phi^4."""

    def __init__(self, kq=3.0):
        self.kq = kq

    def cost(self, free, _p):
        s = _p.obj_scale / _p.num_nodes
        return s * (np.sum((free[_p._slice_v] - 12.) ** 2) + self.kq * np.sum(free[_p._slice_phi] ** 4))

    def cost_grad(self, free, _p):
        s = _p.obj_scale / _p.num_nodes
        g = np.zeros_like(free)
        g[_p._slice_v] = 2 * s * (free[_p._slice_v] - 12.)
        g[_p._slice_phi] = 4 * s * self.kq * free[_p._slice_phi] ** 3
        return g


class exp_comfort(d2oscen.exp_14):
    cost = Comfort()


def _problem_args(N=21):
    g = d2ou.Aircraft()
    ic = (g._sx(0.) - 0., g._sy(0.) - 0., g._spsi(0.) - 0., g._sx(2.) - 20., g._sy(2.) - 5., g._spsi(2.) - 0.)
    bounds = {g._sphi(g._st): (-0.6, 0.6), g._sv(g._st): (9., 15.)}
    return (g.get_eom(d2ou.WindField(w=[0, 0])), g._state_symbols, N, 0.1), dict(known_parameter_map={}, instance_constraints=ic,
                                                                                 bounds=bounds)


def test_problem_from_plain_callables_selects_the_host_objective():
    args, kw = _problem_args()
    N = args[2]
    prob = dc.Problem(lambda x: float(np.sum(x ** 2)), lambda x: 2 * x, *args, **kw)
    assert prob.objective == 'host' and prob.num_free == 5 * N
    np.testing.assert_array_equal(dc.free_index(1, N), np.arange(5 * N).reshape(1, 5, N))


def test_problem_from_an_unknown_plugin_selects_the_host_objective():
    p = sop.Planner(exp_comfort, backend='nlp')
    assert p.prob.objective == 'host' and p.prob.planner is p and p.prob.cost is exp_comfort.cost
    assert p._host_cost
    # the default backend goes to the same Problem (no fit first: the fit cannot express the cost)
    q = sop.Planner(exp_comfort)
    assert q.backend == 'auto' and q._host_cost and q.prob.objective == 'host'
    # a known plug-in keeps its kernel
    assert sop.Planner(d2oscen.exp_14, backend='nlp').prob.objective == 'lowered'
    # and lower_cost itself still knows only the reference's classes
    with pytest.raises(NotImplementedError):
        sop.lower_cost(exp_comfort.cost)


def test_multi_planner_with_an_unknown_plugin_selects_the_host_objective():
    class Sum:
        def __init__(self):
            self.parts = [mop.d2mou.CostInput(vsp=12., kv=5., kphi=1.)]

        def cost(self, free, _p):
            return sum(c.cost(free, _p) for c in self.parts)

        def cost_grad(self, free, _p):
            return sum(c.cost_grad(free, _p) for c in self.parts)

    class scen(mop.exp_5):
        cost, obj_scale = Sum(), 1.0
    p = mop.Planner(scen, backend='nlp')
    assert p.prob.objective == 'host' and p.prob.n_aircraft == 2
    N = p.num_nodes
    idx = dc.free_index(2, N, p)
    np.testing.assert_array_equal(idx, dc.free_index(2, N))               # the planner's slices = the default multi layout
    for a in range(2):
        for c, sl in enumerate((p._slice_x, p._slice_y, p._slice_psi, p._slice_phi, p._slice_v)):
            np.testing.assert_array_equal(idx[a, c], np.arange(5 * 2 * N)[sl[a]])


def test_fit_backend_still_refuses_an_unknown_cost():
    p = sop.Planner(exp_comfort, backend='fit')
    assert not p._host_cost and isinstance(p.prob, sop._FitProblem)
    with pytest.raises(NotImplementedError, match='scalar objective'):
        p.run()


def _synthetic(n, N, kq=0.7, kc=0.3):
    """f = sum_a [ kq sum phi^4 + sum (v_i - v_{i-1})^2 + sum x_i y_i + sum psi_i^2 v_i + kc sum x_i x_{i-2} ] + sum_i x^0_i x^1_i:
    a Hessian that couples nodes one and two apart (inside an aircraft) and the aircraft (outside the blocks)."""
    idx = dc.free_index(n, N)

    def grad(x):
        g = np.zeros_like(x)
        for a in range(n):
            X, Y, P, F, V = (x[idx[a, c]] for c in range(5))
            gX, gY, gP, gF, gV = (np.zeros(N) for _ in range(5))
            gF += 4 * kq * F ** 3
            dv = np.diff(V)
            gV[1:] += 2 * dv; gV[:-1] -= 2 * dv
            gX += Y; gY += X
            gP += 2 * P * V; gV += P ** 2
            gX[2:] += kc * X[:-2]; gX[:-2] += kc * X[2:]
            for c, gc in enumerate((gX, gY, gP, gF, gV)):
                g[idx[a, c]] += gc
        if n >= 2:
            g[idx[0, 0]] += x[idx[1, 0]]; g[idx[1, 0]] += x[idx[0, 0]]
        return g

    def blocks(x):
        H = np.zeros((n, N, 5, 5))
        for a in range(n):
            P, F, V = (x[idx[a, c]] for c in (2, 3, 4))
            H[a, :, 3, 3] = 12 * kq * F ** 2
            H[a, :, 4, 4] = 4.0; H[a, 0, 4, 4] = H[a, -1, 4, 4] = 2.0
            H[a, :, 0, 1] = H[a, :, 1, 0] = 1.0
            H[a, :, 2, 2] = 2 * V
            H[a, :, 2, 4] = H[a, :, 4, 2] = 2 * P
        return H
    return idx, grad, blocks


@pytest.mark.parametrize('n', [1, 2])
def test_curvature_blocks_from_coloured_differences(n):
    N = 23
    idx, grad, blocks = _synthetic(n, N)
    rng = np.random.default_rng(5)
    x = rng.normal(size=5 * N * n) * 3.0
    x[idx[:, 4]] = rng.uniform(9, 15, size=(n, N))
    calls = [0]

    def counted(z):
        calls[0] += 1
        return grad(z)
    g0 = grad(x)
    H = dc.curvature_blocks(counted, x, idx, g0=g0)
    assert calls[0] == 15 * n
    Hx = blocks(x)
    for a in range(n):
        for i in range(N):
            err = np.abs(H[a, i] - Hx[a, i]).max()
            assert err <= 1e-6 * max(1.0, np.abs(Hx[a, i]).max()), (a, i, err)


def test_model_blocks_pack_the_clipped_symmetric_part():
    rng = np.random.default_rng(1)
    H = rng.normal(size=(2, 7, 5, 5))
    Hp = dc.model_blocks(H, 0.25)
    assert Hp.shape == (2, 15, 7)
    S = 0.5 * (H + np.swapaxes(H, -1, -2))
    lam, V = np.linalg.eigh(S)
    ref = (V * np.maximum(lam, 0)[..., None, :]) @ np.swapaxes(V, -1, -2) + 0.25 * np.eye(5)
    k = 0
    for a in range(5):
        for c in range(a, 5):
            np.testing.assert_allclose(Hp[:, k], ref[..., a, c], atol=1e-12)
            k += 1
    # positive semidefinite + sigma: every block's smallest eigenvalue is sigma
    full = np.zeros((2, 7, 5, 5))
    k = 0
    for a in range(5):
        for c in range(a, 5):
            full[..., a, c] = full[..., c, a] = Hp[:, k]
            k += 1
    assert np.linalg.eigvalsh(full).min() >= 0.25 - 1e-12
