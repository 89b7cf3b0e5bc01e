"""CPU: planning in a wind field that varies in space and time -- the host side of d2d_nlp_solve_wind (d2d/wind.py derivatives /
sample_num / sample_sym / negation, the planners' plumbing) and its CPU statement tests/nlp_wind_ref.py, which is arbitrated here by
oracle/nlp.py (a spatially uniform field is a constant wind) and by scipy's SLSQP (a shear)."""
import numpy as np
import pytest
import scipy.optimize

import nlp_wind_ref as R
import wind_ref as WR
from oracle import nlp, costs as C


def test_derivatives_against_central_differences_and_the_planner_protocol():
    """SplineWindField.derivatives against central differences of sample_many with step e = 1e-3 m.
    Bound: a central difference of f has the truncation error e^2/6 |f'''| and the rounding error (error of one evaluation) / e.
    The test fields have amplitudes <= 5 m/s over length scales >= 30 m, so |w'''| <= 5 / 30^3 = 2e-4 and the truncation is
    <= 1e-6 / 6 * 2e-4 = 3e-11; an evaluation sums 64 weighted control points of size <= 6, rounding <= 32 eps * 6 = 4e-14, over
    e: 4e-11.  Together 7e-11: asserted 1e-10 (measured 1e-12 .. 1e-11).  The second derivatives are central differences OF the
    analytic first derivatives (|J| <= 0.2 /s, the same evaluation: rounding 32 eps * 0.2 / e = 1.4e-12; truncation e^2/6 times the
    spline's fourth derivative, zero inside a cell): asserted 1e-10 as well (measured 7e-14).  Points within 2e of a knot
    are kept out (the third derivative jumps there); outside the box the clamped coordinate's derivatives are exactly zero."""
    e = 1e-3
    rng = np.random.default_rng(3)
    for name, F in R.fields().items():
        n = 400
        x = rng.uniform(-149.0, 149.0, n); y = rng.uniform(-199.0, 149.0, n); t = rng.uniform(0.2, 13.8, n)
        keep = (np.abs((x - F.x0) / F.hx - np.round((x - F.x0) / F.hx)) > 2 * e) & (np.abs((y - F.y0) / F.hy - np.round((y - F.y0) / F.hy)) > 2 * e)
        x, y, t = x[keep], y[keep], t[keep]
        assert len(x) > 300
        w, J, H = F.derivatives(t, x, y)
        assert w.shape == (2, len(x)) and J.shape == (2, 2, len(x)) and H.shape == (2, 3, len(x))
        np.testing.assert_array_equal(w, np.stack(F.sample_many(t, x, y)))            # the value IS sample_many's
        dx = (np.stack(F.sample_many(t, x + e, y)) - np.stack(F.sample_many(t, x - e, y))) / (2 * e)
        dy = (np.stack(F.sample_many(t, x, y + e)) - np.stack(F.sample_many(t, x, y - e))) / (2 * e)
        err1 = max(np.abs(J[:, 0] - dx).max(), np.abs(J[:, 1] - dy).max())
        Jxp, Jxm = F.derivatives(t, x + e, y)[1], F.derivatives(t, x - e, y)[1]
        Jyp, Jym = F.derivatives(t, x, y + e)[1], F.derivatives(t, x, y - e)[1]
        err2 = max(np.abs(H[:, 0] - (Jxp[:, 0] - Jxm[:, 0]) / (2 * e)).max(), np.abs(H[:, 1] - (Jyp[:, 0] - Jym[:, 0]) / (2 * e)).max(),
                   np.abs(H[:, 1] - (Jxp[:, 1] - Jxm[:, 1]) / (2 * e)).max(), np.abs(H[:, 2] - (Jyp[:, 1] - Jym[:, 1]) / (2 * e)).max())
        print(f'{name}: first derivatives vs differences {err1:.2e}, second {err2:.2e}')
        assert err1 <= 1e-10 and err2 <= 1e-10, (name, err1, err2)
        assert (np.abs(J).max() > 1e-3) and (name == 'shear' or np.abs(H).max() > 1e-6)       # (the fields do vary)
        # outside the box: the clamped coordinate's derivatives are zero, the other coordinate's are those on the boundary
        xo = np.array([-180.0, 200.0, 20.0, 20.0, -400.0]); yo = np.array([10.0, -30.0, 170.0, -260.0, 300.0]); to = np.full(5, 3.0)
        wo, Jo, Ho = F.derivatives(to, xo, yo)
        np.testing.assert_array_equal(wo, np.stack(F.sample_many(to, xo, yo)))
        assert (Jo[:, 0, [0, 1, 4]] == 0).all() and (Ho[:, 0, [0, 1, 4]] == 0).all() and (Ho[:, 1, :] == 0).all()
        assert (Jo[:, 1, [2, 3, 4]] == 0).all() and (Ho[:, 2, [2, 3, 4]] == 0).all()
        xb = np.clip(xo, -150.0, 150.0); yb = np.clip(yo, -200.0, 150.0)
        _, Jb, _ = F.derivatives(to, xb, yb)
        np.testing.assert_allclose(Jo[:, 1, :2], Jb[:, 1, :2], rtol=0, atol=1e-15)      # d/dy at x outside = d/dy on the boundary
        np.testing.assert_allclose(Jo[:, 0, 2:4], Jb[:, 0, 2:4], rtol=0, atol=1e-15)
        # the planner's protocol
        for tt, xx, yy in ((0.0, 1.0, 2.0), (5.5, -70.0, 33.0), (2.0, 400.0, 0.0)):
            np.testing.assert_array_equal(F.sample_num(tt, xx, yy), F.sample(tt, (xx, yy)))
            np.testing.assert_array_equal((-F).sample(tt, (xx, yy)), -F.sample(tt, (xx, yy)))
        assert (-F).cp.shape == F.cp.shape and ((-F).x0, (-F).hx, (-F).t0, (-F).ht) == (F.x0, F.hx, F.t0, F.ht)


def test_planners_take_a_field_or_say_why_not():
    """Planner(exp) with exp.wind a SplineWindField (exp_14's poses, bounds and cost) builds the collocation problem around the
    field; the fit, a foreign sample_sym class and the multi-aircraft planner refuse by name."""
    import d2d.optyplan_scenarios as d2oscen
    import d2d.opty_utils as d2ou
    import d2d.multiopty_utils as d2mou
    import opty.direct_collocation
    import single_opt_planner as sop
    import multi_opt_planner as mop
    from d2d.wind import SplineWindField
    F = R.fields()['shear']

    class windy(d2oscen.exp_14):
        wind = F
    for backend in (None, 'auto', 'nlp'):
        p = sop.Planner(windy, backend=backend)
        assert isinstance(p.prob, opty.direct_collocation.Problem) and p.prob.field is windy.wind and p.prob.t_start == 0.0
        assert p.prob.objective == 'lowered' and p.prob.num_free == 5 * 121
    eom = p.aircraft.get_eom(F)
    assert eom.field is F and 'wx(t,x,y)' in str(eom) and 'wy(t,x,y)' in str(eom) and len(eom) == 3
    const = p.aircraft.get_eom(d2ou.WindField(w=[1., -2.]))          # a constant class: unchanged
    assert const.field is None and const.wind == (1., -2.) and '+ 1.0' in str(const)
    with pytest.raises(NotImplementedError, match="backend='nlp'"):
        sop.Planner(windy, backend='fit')

    class Foreign:
        def sample_sym(self, t, x, y):
            return [0.1 * y, 0.0]

        def sample_num(self, t, x, y):
            return [0.1 * y, 0.0]

    class foreign(d2oscen.exp_14):
        wind = Foreign()
    with pytest.raises(NotImplementedError, match='from_field'):
        sop.Planner(foreign)
    # ... and from_field takes such a planner wind object (sample_num, no sample)
    G = SplineWindField.from_field(Foreign(), np.arange(-150.0, 151.0, 50.0), np.arange(-150.0, 151.0, 50.0))
    np.testing.assert_allclose(G.sample_num(0.0, 12.0, 40.0), [4.0, 0.0], atol=1e-12)

    class two(mop.trap_4):
        wind = F
    with pytest.raises(NotImplementedError, match='constant wind'):
        mop.Planner(two, backend='nlp')
    with pytest.raises(NotImplementedError, match='one aircraft'):
        acs = d2mou.AircraftSet(n=2)
        cons = tuple(c for ac in acs.aircraft for tt in (0., 4.) for c in (ac._sx(tt) - 0., ac._sy(tt) - 0., ac._spsi(tt) - 0.))
        bounds = {s: (-1., 1.) for ac in acs.aircraft for s in (ac._sphi(acs.st),)}
        bounds.update({ac._sv(acs.st): (9., 15.) for ac in acs.aircraft})
        eom2 = d2ou.Eom(F.sample_sym(None, None, None), ids=(0, 1))
        opty.direct_collocation.Problem(lambda f: 0.0, lambda f: 0 * f, eom2, acs._state_symbols, 41, 0.1, instance_constraints=cons,
                                        bounds=bounds)
    # a field with a host objective: refused when solved
    class Mine:
        def cost(self, free, _p): return float(np.sum(free[_p._slice_v] ** 2))
        def cost_grad(self, free, _p): g = np.zeros_like(free); g[_p._slice_v] = 2 * free[_p._slice_v]; return g

    class host(windy):
        cost = Mine()
    ph = sop.Planner(host)
    assert ph.prob.objective == 'host' and ph.prob.field is F
    with pytest.raises(NotImplementedError, match='host objective'):
        ph.prob.solve(ph.get_initial_guess('tri'))


def test_cpu_statement_in_a_uniform_field_is_the_oracle_in_that_constant_wind():
    """A spline whose control points are all c is the constant wind c: the CPU statement against oracle.nlp.solve from the same 'tri'
    guess at the tolerances tests/test_gpu_nlp.py uses between kernel and oracle."""
    N, h = 41, 0.1
    for c, p1 in (((1.0, -0.5), (46., 5., -0.1, 0., 12.)), ((-2.0, 1.5), (50., -4., 0.3, 0., 12.))):
        p0 = (0., 0., 0.2, 0., 12.)
        kw = dict(vsp=12., kv=5., kphi=1., obj_scale=1., phi_max=np.deg2rad(35.), v_min=9., v_max=15., obstacles=[(24., 1., 5.)], kobs=1.0)
        pbc = nlp.Problem(N, h, p0, p1, wind=c, **kw)
        fp = R.FieldProblem(nlp.Problem(N, h, p0, p1, **kw), R.uniform_field(c), t_start=2.0)
        W0 = nlp.from_free(C.single_guess('tri', p0, p1, 12., (N - 1) * h, N), N)
        Wo, io = nlp.solve(pbc, W0)
        Wf, inf = R.solve(fp, W0)
        print(f'uniform {c}: cost {inf["cost"]:.12f} vs {io["cost"]:.12f}, nodes {np.abs(Wf - Wo).max():.2e}, steps {inf["inner"]} / {io["inner"]}')
        assert io['status'] == 1 and inf['status'] == 1
        assert abs(inf['cost'] - io['cost']) <= 1e-7 * io['cost'] and np.abs(Wf - Wo).max() <= 1e-5
        np.testing.assert_allclose(R.constraints(fp, Wf), nlp.constraints(pbc, Wf), rtol=0, atol=1e-12)


def _arbiter(fp, W0):
    """scipy SLSQP on the same NLP (objective = the one whose gradient is the reference's cost_grad; equalities in the field with
    their analytic Jacobian; the boxes as bounds; the end conditions eliminated) from the same start."""
    pb = fp.pb
    N, h = pb.N, pb.h
    free = ~(pb.lo == pb.hi)
    idx = np.flatnonzero(free.reshape(-1))

    def unpack(z):
        W = np.where(free, 0.0, pb.lo).copy()
        W.reshape(-1)[idx] = z
        return W

    def jac(z):
        W = unpack(z)
        x, y, psi, phi, v = W.T
        _, J, _ = fp.jet(W)
        A = np.zeros((N - 1, 3, N, 5))
        for i in range(1, N):
            k = i - 1
            sp, cp, tp = np.sin(psi[i]), np.cos(psi[i]), np.tan(phi[i])
            A[k, 0, i, 0] = 1 / h + J[0, 0, i]; A[k, 0, i, 1] = J[0, 1, i]; A[k, 0, i, 2] = v[i] * sp; A[k, 0, i, 4] = -cp; A[k, 0, i - 1, 0] = -1 / h
            A[k, 1, i, 0] = J[1, 0, i]; A[k, 1, i, 1] = 1 / h + J[1, 1, i]; A[k, 1, i, 2] = -v[i] * cp; A[k, 1, i, 4] = -sp; A[k, 1, i - 1, 1] = -1 / h
            A[k, 2, i, 2] = 1 / h; A[k, 2, i, 3] = -nlp.G_ACC * (1 + tp * tp) / v[i]; A[k, 2, i, 4] = nlp.G_ACC * tp / v[i] ** 2; A[k, 2, i - 1, 2] = -1 / h
        return A.reshape(3 * (N - 1), 5 * N)[:, idx]

    z0 = np.clip(W0, pb.lo, pb.hi).reshape(-1)[idx]
    r = scipy.optimize.minimize(lambda z: nlp.objective(pb, unpack(z)), z0, jac=lambda z: nlp.cost_grad(pb, unpack(z)).reshape(-1)[idx],
                                method='SLSQP', bounds=list(zip(pb.lo.reshape(-1)[idx], pb.hi.reshape(-1)[idx])),
                                constraints=[dict(type='eq', fun=lambda z: R.constraints(fp, unpack(z)).reshape(-1), jac=jac)],
                                options=dict(ftol=1e-12, maxiter=400))
    return unpack(r.x), r


def test_cpu_statement_in_a_shear_against_scipy_slsqp():
    """31 nodes (3 s, 34 m) in the shear of tests/wind_ref.py, the CPU statement and SLSQP (ftol 1e-12, analytic Jacobians; 36
    iterations, 0.3 s) from the same 'tri' guess.  Measured on the CPU: cost 11.037482613 (statement) vs 11.037482603 (SLSQP), a
    relative gap of 9.14e-10, nodes within 2.9e-6; feasible in the field to 3.0e-10 / 6.7e-14.  Asserted: ten times the measured gap
    (9.2e-9 relative; the arbiter stops at its own ftol) -- tighter than the 1e-5 KKT bar of the existing tests, which is the
    ceiling; the statement's KKT residual in the field <= 1e-5 (measured 7.9e-8)."""
    N, h = 31, 0.1
    p0 = (0., 0., -0.3, 0., 12.); p1 = (34., 3., 0.1, 0., 12.)
    pb = nlp.Problem(N, h, p0, p1, vsp=12., kv=5., kphi=1., obj_scale=1., phi_max=np.deg2rad(35.), v_min=9., v_max=15.)
    fp = R.FieldProblem(pb, R.fields()['shear'], 0.0)
    W0 = nlp.from_free(C.single_guess('tri', p0, p1, 12., (N - 1) * h, N), N)
    W, info = R.solve(fp, W0)
    Ws, r = _arbiter(fp, W0)
    cs = nlp.cost(pb, Ws)
    gap = abs(cs - info['cost']) / info['cost']
    kkt, feas = R.kkt_residual(fp, W, info['mult'], info['zL'], info['zU'])
    fs = float(np.abs(R.constraints(fp, Ws)).max())
    print(f'statement cost {info["cost"]:.12f} feas {info["feas"]:.2e} kkt {kkt:.2e} ({info["inner"]} steps); SLSQP cost {cs:.12f} feas {fs:.2e} '
          f'({r.nit} iterations, status {r.status}); relative gap {gap:.3e}; nodes {np.abs(W - Ws).max():.2e}')
    assert info['status'] == 1 and r.status == 0
    assert info['feas'] <= 1e-8 and feas <= 1e-8 and fs <= 1e-8
    assert gap <= 9.2e-9
    assert kkt <= 1e-5
    # the shear matters on this leg: the same problem in still air has another cost
    assert abs(nlp.solve(pb, W0)[1]['cost'] - info['cost']) > 1e-2 * info['cost']
