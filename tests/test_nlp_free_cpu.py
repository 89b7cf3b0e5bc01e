"""CPU: the statement of the free-time-step collocation solve (tests/nlp_free_ref.py) against the SLSQP arbiter, its own derivatives and
KKT conditions, exp_13 with its duration freed, the cases of the GPU step comparison, and the host lowering of a variable duration.

Measured (the statement against tests/golden/nlp_free_slsqp.npz, 5 cases of 5, 9 and 17 nodes; SLSQP stops at ftol 1e-12, the statement
at opt_tol 1e-7): relative differences, cost / h per case:
  5.0e-10 / 3.7e-10,  1.2e-09 / 6.0e-11,  1.1e-09 / 1.9e-10,  5.5e-09 / 1.0e-11,  2.3e-09 / 5.8e-11
so the tolerances are 10 x the largest: 5.5e-8 on the cost, 3.8e-9 on h.  (Node values are not compared: they are not unique in the
flat directions of the objective)
"""
import os
import re

import numpy as np
import pytest

import nlp_free_ref as F
import nlp_steps_ref as S
from oracle import nlp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'nlp_free_slsqp.npz')
# 10 x the largest relative difference the statement shows over the golden's cases (module docstring)
SLSQP_COST_RTOL = 5.5e-8
SLSQP_H_RTOL = 3.8e-9


def golden_cases():
    g = np.load(GOLDEN)
    for k in range(int(g['n_cases'])):
        N = int(g[f'c{k}_N'])
        fr = g[f'c{k}_free_row']
        fp = F.FreeProblem(nlp.problem_from_row(g[f'c{k}_row'], N, F.H0), fr[0], fr[1], fr[2])
        yield k, fp, g[f'c{k}_W0'], float(g[f'c{k}_cost']), float(g[f'c{k}_h']), float(g[f'c{k}_feas'])


def test_statement_vs_slsqp_golden():
    worst_c = worst_h = 0.0
    for k, fp, W0, cost, h, feas in golden_cases():
        W, info = F.solve(fp, W0, F.H0)
        dc, dh = abs(info['cost'] - cost) / cost, abs(info['h'] - h) / h
        worst_c, worst_h = max(worst_c, dc), max(worst_h, dh)
        print(f'case {k} (N {fp.pb.N}): status {info["status"]}, {info["inner"]} steps, cost off by {dc:.2e} relative, h by {dh:.2e} relative')
        assert info['status'] == 1 and info['feas'] <= 1e-9 and feas <= 1e-9
        assert dc <= SLSQP_COST_RTOL and dh <= SLSQP_H_RTOL
    print(f'largest: cost {worst_c:.2e}, h {worst_h:.2e}')


def test_h_row_matches_central_differences_of_the_merit():
    """Gradient g_u, curvature d_u and border column b of the statement against central differences of its own augmented-Lagrangian
    value at a random interior point.  Step e = 1e-5 on values of order 10: first differences carry e^2 |f'''| / 6 + eps |f| / e ~ 1e-8
    relative of the largest entry, the mixed second differences eps |f| / e^2 ~ 1e-16 * 1e5 / 1e-10 = 1e-1 absolute on entries up to
    1e3 * rho: the tolerances are 1e-6 and 1e-3 of the largest entry."""
    fp, _, W0 = F.leg_problem(17, 0, obstacle=1, k_dur=0.5)
    pb = fp.pb
    fixed, _, _ = nlp._barrier_sets(pb)
    rng = np.random.default_rng(0)
    W = W0.copy(); W[:, 3] = rng.uniform(-0.3, 0.3, 17); W[:, 4] = rng.uniform(10, 14, 17); W[fixed] = pb.lo[fixed]
    u, mu, rho = 9.3, 0.1 * rng.standard_normal((16, 3)), 10.0
    g, D, E, g_u, b, d_u = fp.normal_equations(W, u, mu, rho)
    al = lambda W, u: nlp._al_value(fp.at(u), W, mu, rho) + fp.duration_cost(u)      # noqa: E731
    e = 1e-5
    fd_g = (al(W, u + e) - al(W, u - e)) / (2 * e)
    assert abs(2 * g_u - fd_g) <= 1e-6 * abs(fd_g), (2 * g_u, fd_g)
    e2 = 1e-3                                      # (the pure second difference: a larger step, the function is quadratic in u but for k / u)
    fd_d = (al(W, u + e2) - 2 * al(W, u) + al(W, u - e2)) / e2 ** 2
    assert abs(2 * d_u - fd_d) <= 1e-5 * abs(fd_d), (2 * d_u, fd_d)
    bb = np.zeros_like(b)
    e3 = 1e-4
    for i in range(17):
        for c in range(5):
            Wp = W.copy(); Wp[i, c] += e3; Wm = W.copy(); Wm[i, c] -= e3
            bb[i, c] = (al(Wp, u + e3) - al(Wp, u - e3) - al(Wm, u + e3) + al(Wm, u - e3)) / (4 * e3 * e3)
    free = ~fixed
    err = np.abs(np.where(free, 2 * b - bb, 0.0)).max()
    print(f'border: largest entry {np.abs(bb).max():.3e}, largest difference {err:.2e}')
    assert err <= 1e-3 * np.abs(bb).max()
    # the node gradient at this u is oracle.nlp's (the statement reuses it): one entry as a cross check
    Wp = W.copy(); Wp[5, 2] += e; Wm = W.copy(); Wm[5, 2] -= e
    assert abs(2 * g[5, 2] - (al(Wp, u) - al(Wm, u)) / (2 * e)) <= 1e-6 * abs(2 * g[5, 2])


def test_kkt_residual_with_the_h_row_at_the_solutions():
    """Stationarity of the Lagrangian on the node rows AND the row of u, at most 1e-6, with the multipliers the last inner problem is
    stationary with, 2 rho (mu + c).  (With 2 rho mu, the estimate that inner problem started from, the residual carries 2 rho J^T c:
    measured 9e-9 .. 2.7e-6 over these cases against 7e-11 .. 4e-8.)"""
    worst = 0.0
    cases = [(fp, W0) for _, fp, W0, *_ in golden_cases()] + [F.leg_problem(41, 300, k_dur=0.5)[::2], F.leg_problem(41, 300, k_dur=0.5, obstacle=1)[::2]]
    for fp, W0 in cases:
        W, info = F.solve(fp, W0, F.H0)
        kkt, feas = F.kkt_residual(fp, W, info['h'], info['mult_last'], info['zL'], info['zU'], info['zu'])
        worst = max(worst, kkt)
        assert info['status'] == 1 and kkt <= 1e-6 and feas <= 1e-9, (fp.pb.N, kkt, feas)
    print(f'largest KKT residual {worst:.2e}')


def _exp13_problem():
    import d2d.optyplan_scenarios as sc
    import d2d.opty_utils as ou
    import single_opt_planner as sop
    e = sc.exp_13
    N, h, dur = ou.planner_timing(e.t0, e.t1, e.hz)
    row = sop.scen_row(e.p0, e.p1, e.vref, sop.lower_cost(e.cost), e.obj_scale / N, e.wind.w, e.phi_constraint, e.v_constraint)
    W0 = np.stack(ou.triangle(e.p0[:2], e.p1[:2], e.vref, dur, N, go_left=-1.), 1)
    return nlp.problem_from_row(row, N, h), W0, N, h


def test_exp13_with_a_free_duration():
    """exp_13 asks for a quarter turn in 3.0 s that needs 3.3 s at least: with t1 free in (2, 6) s the statement
    converges to a duration >= 3.3 s, with the step fixed it stays STALLED."""
    pb, W0, N, h = _exp13_problem()
    fp = F.FreeProblem(pb, 2.0 / (N - 1), 6.0 / (N - 1), 0.0)
    W, info = F.solve(fp, W0, h)
    print(f'exp_13 free: status {info["status"]}, duration {info["h"] * (N - 1)!r}, cost {info["cost"]!r}, feas {info["feas"]:.1e}')
    assert info['status'] == 1 and info['h'] * (N - 1) >= 3.3 and info['feas'] <= 1e-9
    assert nlp.solve(pb, W0)[1]['status'] == 4


@pytest.mark.parametrize('lid', [str(N) for N in F.STEP_N] + ['bounds'])
def test_step_cases_are_determined(lid):
    """Every case of the GPU step comparison, on the statement alone (nlp_steps_ref.check): its tolerance is at most 1e-8 and the
    perturbed starts take the same path after every budget; budgets with outer_max = 1 end at 'max iterations' with every step
    accepted.  The 3-node disc and box cases solve their first inner problem within 8 steps, so for them the budget (8, 1) is held to
    the first two checks only."""
    cases = F.bounds_launch()[0] if lid == 'bounds' else F.steps_launch(int(lid))[0]
    for case in cases:
        for budget in S.BUDGETS:
            bad = S.check(case, budget)
            if lid == '3' and budget == (8, 1):
                bad = [b for b in bad if b.startswith('tol') or b.startswith('the perturbed')]
            assert not bad, (case.cid, budget, bad)
    if lid == 'bounds':                          # the third case: h_lo 5 % above the interior optimum of the same row
        fr = F.bounds_launch()[2]
        (W0, h_start) = _hlo_start()
        _, info = F.solve(_hlo_problem(), W0, h_start)
        assert info['status'] == 1 and fr[2, 0] < info['h'] <= fr[2, 0] * (1 + 1e-6), (info['h'], fr[2, 0])


def _hlo_problem():
    cases, rows, fr, _ = F.bounds_launch()
    return F.FreeProblem(nlp.problem_from_row(rows[2], 41, F.H0), fr[2, 0], fr[2, 1], fr[2, 2])


def _hlo_start():
    cases, rows, fr, _ = F.bounds_launch()
    return cases[2].W0[0][:-1], fr[2, 3]


# ---- host lowering ------------------------------------------------------------------------------------------------------------------
def _planner(exp, **kw):
    import single_opt_planner as sop
    return sop.Planner(exp, **kw)


def _exp13(**attrs):
    import d2d.optyplan_scenarios as sc
    return type('exp_13_v', (sc.exp_13,), attrs)


def test_problem_with_a_symbol_interval():
    import sympy
    import opty.direct_collocation as odc
    import d2d.opty_utils as ou
    p = _planner(_exp13(t1_free=(2.0, 6.0)))
    assert p.prob.num_free == 5 * 31 + 1 and p.prob.objective == 'lowered'
    assert p.prob.step_bounds == (2.0 / 30, 6.0 / 30)
    assert p.get_initial_guess()[-1] == 0.1
    q = _planner(_exp13(), backend='nlp')
    g, e = q.aircraft, _exp13()
    cost = e.cost                                # (the closures hold the plug-in itself, as the reference's call sites do)
    bounds = {g._sphi(g._st): e.phi_constraint, g._sv(g._st): e.v_constraint}
    mk = lambda h, b=None, ic=None, eom=None, **kw: odc.Problem(lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q),     # noqa: E731
                                                               eom or g.get_eom(e.wind), g._state_symbols, 31, h, known_parameter_map={},
                                                               instance_constraints=ic or q._instance_constraints, bounds=b or bounds, **kw)
    h = sympy.Symbol('h')
    pr = mk(h, {**bounds, h: (0.07, 0.15)})
    assert pr.num_free == 156 and pr.step_bounds == (0.07, 0.15)
    assert mk(h).step_bounds is None and mk(ou._Sym('h')).num_free == 156 and mk(0.1).num_free == 155
    with pytest.raises(ValueError, match='time step'):
        mk(h, {**bounds, h: (0.15, 0.07)})
    # each unsupported combination by name
    with pytest.raises(NotImplementedError, match='interior times'):
        mk(h, ic=q._instance_constraints + (g._sx(1.0) - 80.0,))
    from d2d.wind import SplineWindField
    fld = SplineWindField(np.zeros((2, 11, 11)), -200.0, 50.0, -200.0, 50.0)
    with pytest.raises(NotImplementedError, match='wind field'):
        mk(h, eom=g.get_eom(fld))
    with pytest.raises(NotImplementedError, match='host objective'):
        odc.Problem(lambda f: 0.0, lambda f: np.zeros_like(f), g.get_eom(e.wind), g._state_symbols, 31, h, instance_constraints=q._instance_constraints, bounds=bounds)
    mov = _planner(_exp13(moving_obstacles=[ou.MovingObstacle.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), backend='nlp')
    with pytest.raises(NotImplementedError, match='moving obstacles'):
        odc.Problem(lambda f: cost.cost(f, mov), lambda f: cost.cost_grad(f, mov), g.get_eom(e.wind), g._state_symbols, 31, h,
                    instance_constraints=q._instance_constraints, bounds=bounds)
    g2 = [ou.Aircraft(id='_0'), ou.Aircraft(id='_1')]
    with pytest.raises(NotImplementedError, match='more than one aircraft'):
        ic = tuple(s(t) - 0.0 for a in g2 for s in (a._sx, a._sy, a._spsi) for t in (0.0, 3.0))
        b2 = {a._sphi(a._st): e.phi_constraint for a in g2}; b2.update({a._sv(a._st): e.v_constraint for a in g2})
        odc.Problem(lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q), ou.Eom((0.0, 0.0), ids=('_0', '_1')),
                    g2[0]._state_symbols + g2[1]._state_symbols, 31, h, instance_constraints=ic, bounds=b2)


def test_cost_duration_and_composit_lowering():
    import d2d.opty_utils as ou
    import single_opt_planner as sop
    p = _planner(_exp13(t1_free=(2.0, 6.0)))
    free = np.concatenate([np.arange(155.0), [0.11]])
    c = ou.CostDuration(0.7)
    assert c.cost(free, p) == 0.7 * 30 * 0.11
    g = c.cost_grad(free, p)
    assert g.shape == free.shape and not g[:-1].any() and g[-1] == 0.7 * 30
    assert not c.cost_grad(free[:-1], p).any() and c.cost(free[:-1], p) == 0.7 * 30 * p.time_step
    low = sop.lower_cost(c)
    assert len(low) == 9 and sop.duration_weight(low) == 0.7 and low[:5] == (0., 0., 0., 0., ())
    obss = [(30.0, 0.0, 5.0)]
    old = sop.lower_cost(ou.CostComposit(obss, vsp=12.0, kobs=2.0, kvel=3.0, kbank=0.5, obs_kind=1))
    new = sop.lower_cost(ou.CostComposit(obss, vsp=12.0, kobs=2.0, kvel=3.0, kbank=0.5, obs_kind=1, kdur=0.25))
    assert type(old) is tuple and sop.duration_weight(old) == 0.0            # without kdur: the plain tuple of before
    assert repr(tuple(new)) == repr(old) and sop.duration_weight(new) == 0.25
    cc = ou.CostComposit(None, vsp=12.0, kdur=0.25)
    assert abs(cc.cost(free, p) - (ou.CostComposit(None, vsp=12.0).cost(free, p) + 0.25 * 30 * 0.11)) <= 1e-12
    assert cc.cost_grad(free, p)[-1] == 0.25 * 30
    # the scenario row does not see the duration weight: byte for byte the row of the cost without it
    r_old = sop.scen_row((0, 0, 0, 0, 12), (10, 0, 0, 0, 12), 12.0, old, 0.1, (0.0, 0.0), (-0.5, 0.5), (9.0, 15.0))
    r_new = sop.scen_row((0, 0, 0, 0, 12), (10, 0, 0, 0, 12), 12.0, new, 0.1, (0.0, 0.0), (-0.5, 0.5), (9.0, 15.0))
    assert r_old.tobytes() == r_new.tobytes()


def test_t1_free_is_validated():
    for bad in ((4.0, 2.0), (0.0, 3.0), (-1.0, 3.0), (3.0, 3.0), (2.0, np.inf)):
        with pytest.raises(ValueError, match='t1_free'):
            _planner(_exp13(t1_free=bad))
    with pytest.raises(NotImplementedError, match="backend='fit'"):
        _planner(_exp13(t1_free=(2.0, 6.0)), backend='fit')
    import single_opt_planner as sop
    assert isinstance(_planner(_exp13(t1_free=(2.0, 6.0)), backend='auto').prob, __import__('opty.direct_collocation').direct_collocation.Problem)
    assert isinstance(_planner(_exp13()).prob, sop._FitProblem)               # without it the scenario plans as before


def test_plan_batch_refuses_by_name():
    import full_sim
    rows, W0 = np.zeros((2, 64)), np.zeros((2, 5, 41))
    with pytest.raises(NotImplementedError, match='n_ac > 1'):
        full_sim.plan_batch(rows, 41, 4.0, 1.0 / 41, backend='nlp', W0=W0, h=0.1, n_ac=2, free_time=(0.05, 0.2))
    with pytest.raises(NotImplementedError, match='polynomial fit'):
        full_sim.plan_batch(rows, 41, 4.0, 1.0 / 41, backend='fit', free_time=(0.05, 0.2))


def test_header_version():
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 120
    assert 'd2d_nlp_solve_free' in hdr and 'd2d_nlp_free_workspace_doubles' in hdr
