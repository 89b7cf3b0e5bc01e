"""CPU: the statement of the collocation solve with a FREE time step outside static hard discs and inside a convex polygon
(tests/nlp_free_fence_ref.py; include/d2d.h d2d_nlp_solve_free_fence), and the host layers that route to it, without a device.

Against the SLSQP arbiter tests/golden/nlp_free_fence_slsqp.npz (scipy SLSQP over the node values and h itself, the discs and the edges
as inequality constraints; 5, 9 and 17 nodes, a disc or an edge active at every optimum).  Measured on the statement, relative:
    case        cost gap    h gap      steps   largest dual (disc / edge)
    cut-5       4.06e-09    8.06e-10   21      - / 2.09
    cut-9       3.99e-09    8.79e-10   28      - / 6.29
    disc-17     2.00e-09    2.74e-11   37      7.31 / -
    cut-17      3.18e-09    4.86e-13   35      - / 1.19
    mixed-17    5.70e-10    7.48e-10   40      76.3 / 38.3
The bounds asserted are 10 x what the neighbours hold their own goldens to: cost 10 x 5.5e-8 (tests/test_nlp_free_cpu.py; tests/
test_nlp_fence_cpu.py holds 8.4e-8: the smaller of the two is taken), h 10 x 3.8e-9 (tests/test_nlp_free_cpu.py; the fence golden has
no h).  The measured gaps use 0.7 % and 2.3 % of them.

The step-case table (nlp_free_fence_ref.STEP_CASES), chosen with tools/dev/nlp_free_fence_select.py.  31 of the 32 cells have a
candidate that is determined within nlp_steps_ref.TOL_CAP, keeps stepping after every budget and -- where something can bind -- reaches
a dual of 1 inside the budgets ('many' holds only rows that are far away, as nlp_keepout_ref's 'many' does: nothing there can bind, so
it is not asked for the dual; its largest is 0.045):
    nodes   disc        edge        both        many
    3       (0.09, 5)   -           (0.08, 10)  (0.09, 5)
    5       (0.06, 8)   (0.09, 2)   (0.06, 4)   (0.09, 0)
    17      (0.07, 5)   (0.09, 2)   (0.07, 13)  (0.09, 0)
    64      (0.07, 1)   (0.09, 0)   (0.06, 6)   (0.09, 2)
    65      (0.06, 7)   (0.09, 2)   (0.07, 2)   (0.09, 0)
    121     (0.09, 0)   (0.09, 0)   (0.09, 7)   (0.09, 9)
    122     (0.09, 4)   (0.09, 0)   (0.09, 2)   (0.09, 2)
    129     (0.09, 11)  (0.09, 3)   (0.09, 0)   (0.09, 1)
Both conditions hold: every node count keeps three kinds or four, every kind survives at seven node counts or more.
What the 'edge' kind took.  A convex set that holds both end poses holds the leg's axis, so an edge cannot be laid across the leg as a
disc can; it binds only where the end headings bow the plan.  A rectangle with ONE long edge at half the free plan's bow and the others
far off (the geometry of nlp_fence_ref's step cases) is determined and keeps stepping at every node count, but its dual stays below 1
inside the budgets' 20 Newton steps from 64 nodes on -- 0.07 .. 0.64 at 64 nodes, 0.04 .. 0.21 at 121 .. 129, also with the edge at 30,
20, 10 and 2 % of the bow (0.39) and with the objective scaled by 10 and 100 (0.74): GeoFence's kap, where the start rule puts a node,
is 1 % of the polygon's width, metres there, and the duals start at mub / kap.  A corridor in earnest -- BOTH long edges at half the bow
-- has a kap of centimetres: the largest dual inside the budgets is 10 .. 26 at 64 .. 129 nodes (931 at 5) and rises over the first
budgets (5.9, 6.0, 8.6, 11.4 at 64 nodes), i.e. the edge pushes and is not only started high.  That is the kind's geometry now
(step_corridor(narrow=True)).  The one cell without a candidate is 'edge' at 3 nodes: with one free node the plan without tables has no
bow to cut, or the case converges inside a budget.
"""
import os
import re

import numpy as np
import pytest

import nlp_fence_ref as E
import nlp_free_fence_ref as FF
import nlp_free_ref as F
import nlp_keepout_ref as K
import nlp_steps_ref as S
from oracle import nlp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'nlp_free_fence_slsqp.npz')
SLSQP_COST_RTOL = 10 * 5.5e-8
SLSQP_H_RTOL = 10 * 3.8e-9


@pytest.fixture(scope='module')
def arbiter_solves():
    g = np.load(GOLDEN)
    out = []
    for k in range(int(g['n_cases'])):
        name = str(g[f'c{k}_name'])
        fp, row, W0, discs, edges = FF.arbiter_problem(name)
        assert np.array_equal(row, g[f'c{k}_row']) and np.array_equal(W0, g[f'c{k}_W0']) and np.array_equal(discs, g[f'c{k}_discs'])
        assert np.array_equal(edges, g[f'c{k}_edges']) and np.array_equal(g[f'c{k}_free_row'], [fp.h_lo, fp.h_hi, fp.k_dur, 0.0])
        out.append((name, fp, discs, edges, FF.solve(fp, W0, FF.H0, discs, edges), float(g[f'c{k}_cost']), float(g[f'c{k}_h']), float(g[f'c{k}_gmin'])))
    return out


def test_statement_vs_slsqp_golden(arbiter_solves):
    assert sorted({fp.pb.N for _, fp, *_ in arbiter_solves}) == [5, 9, 17]
    for name, fp, discs, edges, (W, info), cost, h, gmin in arbiter_solves:
        dc, dh = abs(info['cost'] - cost) / cost, abs(info['h'] - h) / h
        print(f'{name}: status {info["status"]}, {info["inner"]} steps, cost off by {dc:.2e} relative, h by {dh:.2e}, duals {info["zk"].max(initial=0):.3g} / '
              f'{info["zf"].max(initial=0):.3g}')
        assert info['status'] == 1 and fp.h_lo < info['h'] < fp.h_hi
        assert dc <= SLSQP_COST_RTOL and dh <= SLSQP_H_RTOL
        assert -1e-9 <= gmin <= 1e-7                                     # a disc or an edge is active at SLSQP's optimum
        assert max(info['zk'].max(initial=0.0), info['zf'].max(initial=0.0)) > 1.0       # and carries a multiplier at the statement's


def test_kkt_residual_at_a_converged_solve(arbiter_solves):
    """Stationarity with the multipliers the last inner problem is stationary with, the row of u and both families' terms included, and
    both families' complementarity |z g - mub| <= 1e-12 max(1, z g) (measured: at most 7.8e-14 over the five cases, mub = 1e-9)."""
    for name, fp, discs, edges, (W, info), *_ in arbiter_solves:
        stat, feas = FF.kkt_residual(fp, W, info, discs, edges)
        print(f'{name}: stationarity {stat:.2e}, feasibility {feas:.2e}')
        assert feas <= nlp.FEAS_TOL and stat <= 1e-6
        mub = info['mub']
        if len(discs):
            zg = info['zk'][:, 1:-1] * K.g_values(W[1:-1], discs)[0]
            assert np.abs(zg - mub).max() <= 1e-12 * max(1.0, float(zg.max()))
            assert (K.g_values(W[1:-1], discs)[0] > 0).all() and not info['zk'][:, [0, -1]].any()
        if len(edges):
            zg = info['zf'][:, 1:-1] * E.g_values(W[1:-1], edges)
            assert np.abs(zg - mub).max() <= 1e-12 * max(1.0, float(zg.max()))
            assert (E.g_values(W[1:-1], edges) > 0).all() and not info['zf'][:, [0, -1]].any()
        # the row of u on its own: d/du [k_dur (N - 1) / u + mult . c] - zu_lower + zu_upper
        u = info['u']
        dl = W[1:, :3] - W[:-1, :3]
        su = -fp.k_dur * (fp.pb.N - 1) / (u * u) + float(np.sum(info['mult_last'] * dl)) - info['zu'][0] + info['zu'][1]
        assert abs(su) <= 1e-6


@pytest.mark.parametrize('N,seed', FF.VERIFIED)
def test_only_the_free_step_answers(N, seed):
    """The two verified cases: the detour round the disc does not fit (N - 1) h seconds at h = 0.1 -- the fixed step STALLS -- and the free
    step CONVERGES with h strictly inside its box and every g > 0."""
    fp, r, W0, discs, edges = FF.detour_problem(N, seed)
    _, fixed = FF.fixed_solve(fp, W0, FF.H0, discs, edges)
    W, info = FF.solve(fp, W0, FF.H0, discs, edges)
    print(f'{N}/{seed}: fixed status {fixed["status"]} feas {fixed["feas"]:.2f} after {fixed["inner"]} steps; free status {info["status"]} after {info["inner"]}, '
          f'h {info["h"]:.5f}, smallest g {min(K.g_values(W[1:-1], discs[discs[:, 2] > 0])[0].min(), E.g_values(W[1:-1], edges[E.present(edges)]).min()):.1e}')
    assert fixed['status'] == 4 and info['status'] == 1
    assert fp.h_lo < info['h'] < fp.h_hi and info['feas'] <= nlp.FEAS_TOL
    assert (K.g_values(W[1:-1], discs[discs[:, 2] > 0])[0] > 0).all() and (E.g_values(W[1:-1], edges[E.present(edges)]) > 0).all()
    assert info['zk'].max() > 1e-2


def test_no_tables_is_the_free_statement_bit_for_bit():
    for N, seed, kw in ((17, 3, dict(k_dur=0.5)), (41, 1, dict(k_dur=2.0, box=True))):
        fp, r, W0 = F.leg_problem(N, seed, **kw)
        Wa, ia = FF.solve(fp, W0, FF.H0, np.zeros((0, 3)), np.zeros((0, 4)))
        Wb, ib = F.solve(fp, W0, FF.H0)
        assert np.array_equal(Wa, Wb)
        for k, v in ib.items():
            assert np.array_equal(np.asarray(ia[k], dtype=object if k == 'path' else None), np.asarray(v, dtype=object if k == 'path' else None)), k
        assert ia['zk'].shape == (0, N) and ia['zf'].shape == (0, N)


def test_refusals_of_the_statement():
    fp, r, W0, discs, edges = FF.detour_problem(17, 0)
    bad_edge = edges.copy(); bad_edge[0, :2] *= 1.0 + 1e-9              # |a| off 1
    inside = discs.copy(); inside[0, :2] = fp.pb.p1[:2]                   # an end pose inside a disc
    for d, e in ((discs, bad_edge), (inside, edges)):
        W, info = FF.solve(fp, W0, FF.H0, d, e)
        assert info['status'] == FF.ST_NONFINITE and np.isnan(info['cost']) and np.isnan(info['h']) and np.array_equal(W, W0)


def test_step_table_meets_the_conditions():
    """The issue's two conditions on STEP_CASES: every node count keeps at least three of its four kinds, and each kind survives at five
    node counts or more (the module docstring has the table)."""
    per_n = {N: [t for t in FF.STEP_TAGS if (N, t) in FF.STEP_CASES] for N in FF.STEP_N}
    per_tag = {t: [N for N in FF.STEP_N if (N, t) in FF.STEP_CASES] for t in FF.STEP_TAGS}
    print(per_n, per_tag)
    assert all(len(v) >= 3 for v in per_n.values()), per_n
    assert all(len(v) >= 5 for v in per_tag.values()), per_tag


@pytest.mark.parametrize('N', FF.STEP_N)
def test_step_cases_are_determined(N):
    """Every LISTED case of the GPU step comparison, on the statement alone: determined within nlp_steps_ref.TOL_CAP with the perturbed
    starts on the same path, still stepping after every budget (3 and 5 nodes: the budget (8, 1) is held to the first two, as in the
    neighbours), and a dual of a disc or an edge of at least 1 inside the budgets ('many': every present row far away, nothing binds)."""
    launch = FF.steps_launch(N)
    assert launch
    for tag, (case, r, discs, edges, fp) in launch.items():
        zmax = 0.0
        for budget in S.BUDGETS:
            assert not FF.step_complaints(case, N, budget), (case.cid, budget)
            raw = S.measure(case, budget)['info']['raw']
            zmax = max(zmax, float(raw['zk'].max(initial=0.0)), float(raw['zf'].max(initial=0.0)))
        assert zmax >= 1.0 or tag == 'many', (case.cid, zmax)
        assert fp.k_dur == FF.STEP_KDUR[tag]
        if tag == 'many':
            assert (discs[:, 2] > 0).sum() == FF.MAX_KEEP - 2 and E.present(edges).sum() == FF.MAX_FENCE - 2 and zmax < 0.1
        if tag == 'both':
            assert np.isfinite(fp.pb.lo[1, 1]) and (discs[:, 2] > 0).sum() == 1 and E.present(edges).sum() == 4


def test_full_cases_converge_with_a_binding_constraint():
    for N in (17, 41):                                                    # (121 nodes: the same rule, run by tools/dev/nlp_free_fence_select.py)
        got = FF.full_launch(N)
        assert len(got) == 8
        for b, (fp, r, W0, discs, edges) in enumerate(got[:3]):
            W, info = FF.solve(fp, W0, FF.H0, discs, edges)
            assert info['status'] == 1 and fp.h_lo < info['h'] < fp.h_hi
            assert max(info['zk'].max(initial=0.0), info['zf'].max(initial=0.0)) > 1e-4


# ---- host logic, no device ----------------------------------------------------------------------------------------------------------
def test_header_version_and_export():
    import d2dhip
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 129
    assert re.search(r'\bint d2d_nlp_solve_free_fence\(', hdr) and 'tests/nlp_free_fence_ref.py' in hdr
    assert 'd2d_nlp_solve_free_fence' in d2dhip.EXPORTS
    assert len(d2dhip._SIGS['d2d_nlp_solve_free_fence'][1]) == 19


def test_nlp_plan_window_routes_and_refuses_by_name():
    import d2dhip

    class _Stub:
        def nlp_solve_free_fence(self, scen, W, h, free_rows, **kw):
            return dict(args=(scen, W, h, free_rows), kw=kw)
    out = d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, window='R', keep='K', fence='E', inner_max=7)
    assert out['entry'] == 'nlp_solve_free_fence' and out['args'] == ('S', 'W', 0.1, 'R') and out['kw'] == dict(discs='K', edges='E', inner_max=7)
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, window='R')['kw'] == dict(discs=None, edges=None)
    for kw, name in ((dict(n_ac=2), 'n_ac'), (dict(field='x'), 'field'), (dict(via='x'), 'via'), (dict(knots='x'), 'knots'), (dict(disc='x'), 'disc'),
                     (dict(hard_knots='x', hard_disc='y'), 'hard_knots'), (dict(free_rows='x'), 'free_rows')):
        with pytest.raises(NotImplementedError, match=f'window together with {name}'):
            d2dhip.nlp_plan(None, None, None, 0.1, window='R', **kw)
    # the old spelling keeps refusing, read from the running code
    with pytest.raises(NotImplementedError, match='keep together with free_rows'):
        d2dhip.nlp_plan(None, None, None, 0.1, free_rows='R', keep='K')
    with pytest.raises(NotImplementedError, match='fence together with free_rows'):
        d2dhip.nlp_plan(None, None, None, 0.1, free_rows='R', fence='E')


def test_plan_batch_window_refuses_by_name():
    import d2d.opty_utils as ou
    import full_sim
    from d2d.wind import SplineWindField
    rows = np.zeros((2, 4))                      # (place holders: every refusal comes before the rows are read)
    kw0 = dict(backend='nlp', W0=np.zeros((2, 5, 17)), h=0.1, window=(0.05, 0.2))
    with pytest.raises(NotImplementedError, match='fit backend'):
        full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, backend='fit', window=(0.05, 0.2))
    mk = ou.MovingKeepOut.linear((0.0, 0.0), (1.0, 0.0), 1.0)
    for kw, name in ((dict(n_ac=2), 'n_ac > 1'), (dict(moving=[ou.MovingObstacle((0.0, 1.0), ((0.0, 0.0), (1.0, 0.0)), 1.0)]), 'moving'),
                     (dict(via=[[], []]), 'via'), (dict(hard_moving=[mk]), 'hard_moving'), (dict(free_time=(0.05, 0.2)), 'free_time'),
                     (dict(deconflict=dict(d_sep=4.0, margin=1.0, d_look=50.0)), 'deconflict')):
        with pytest.raises(NotImplementedError, match=f'window with {name} is not supported'):
            full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, **kw0, **kw)
    fld = SplineWindField(np.zeros((2, 11, 11)), -200.0, 50.0, -200.0, 50.0)
    with pytest.raises(NotImplementedError, match='window with windfield is not supported'):
        full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, windfield=fld, **kw0)
    # the old spellings keep refusing, read from the running code
    with pytest.raises(NotImplementedError, match='keep_out with free_time is not supported'):
        full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, backend='nlp', W0=np.zeros((2, 5, 17)), h=0.1, free_time=(0.05, 0.2), keep_out=np.zeros((2, 1, 3)))


def _exp14(**attrs):
    import d2d.optyplan_scenarios as sc
    return type('exp_14_w', (sc.exp_14,), attrs)


def test_planner_window_lowers_with_h_hi_and_refuses_by_name():
    import d2d.optyplan_scenarios as sc
    import d2d.opty_utils as ou
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    from test_nlp_fence_cpu import scenario_fence
    t0, t1 = sc.exp_14.t0, sc.exp_14.t1
    win = (t1 - 2.0, t1 + 6.0)
    ko = ou.KeepOut((2.88, -4.54), 5.0, margin=1.0)
    gf = scenario_fence(sc.exp_14, 50.0, 50.0, 1.0)
    p = sop.Planner(_exp14(keep_out=[ko], fence=gf, t1_window=win), backend='auto')      # 'auto' goes straight to the collocation backend
    assert isinstance(p.prob, odc.Problem) and p.prob.free_step is not None and p.t1_window == win and p.t1_free is None
    h_lo, h_hi = ((t - t0) / (p.num_nodes - 1) for t in win)
    assert p.prob.step_bounds == (h_lo, h_hi)
    assert p.prob.keep_rows[0, 2] == K.lowered_radius(5.0, 1.0, sc.exp_14.v_constraint[1], h_hi)        # the LARGEST step of the window
    assert p.prob.keep_rows[0, 2] > K.lowered_radius(5.0, 1.0, sc.exp_14.v_constraint[1], p.time_step)
    assert np.array_equal(p.prob.fence_rows, gf.lowered()) and p.prob.num_free == 5 * p.num_nodes + 1
    assert p.get_initial_guess()[-1] == p.time_step
    # without discs or fence: the Problem of t1_free, argument for argument
    a, b = sop.Planner(_exp14(t1_window=win), backend='nlp'), sop.Planner(_exp14(t1_free=win), backend='nlp')
    assert a.prob.step_bounds == b.prob.step_bounds and not a.prob.keep_out and a.prob.fence is None and a.prob.num_free == b.prob.num_free
    with pytest.raises(NotImplementedError, match="backend='fit' cannot plan with a free duration"):
        sop.Planner(_exp14(t1_window=win), backend='fit')
    with pytest.raises(ValueError, match='t1_window'):
        sop.Planner(_exp14(t1_window=(t1 + 1.0, t1)), backend='nlp')
    from d2d.wind import SplineWindField
    fld = SplineWindField(np.zeros((2, 11, 11)), -200.0, 50.0, -200.0, 50.0)
    for attrs, name in ((dict(t1_free=win), 't1_free'), (dict(moving_obstacles=[ou.MovingObstacle.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), 'moving obstacles'),
                        (dict(waypoints=[ou.Waypoint(t0 + 1.0, x=1.0)]), 'waypoints'),
                        (dict(keep_out=[ou.MovingKeepOut.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), 'a MovingKeepOut'),
                        (dict(wind=fld), 'a wind field')):
        with pytest.raises(NotImplementedError, match=f't1_window together with {name}'):
            sop.Planner(_exp14(t1_window=win, **attrs), backend='nlp')
    # the old spelling keeps refusing, read from the running code
    with pytest.raises(NotImplementedError, match='keep_out together with a free duration'):
        sop.Planner(_exp14(keep_out=[ko], t1_free=win), backend='nlp')
    with pytest.raises(NotImplementedError, match='fence together with a free duration'):
        sop.Planner(_exp14(fence=gf, t1_free=win), backend='nlp')
    # the upstream spelling needs the bound of the step for the lowering
    q = sop.Planner(_exp14(), backend='nlp')
    e, g = _exp14(), q.aircraft
    h = ou._Sym('h')
    bounds = {g._sphi(g._st): e.phi_constraint, g._sv(g._st): e.v_constraint}
    cost = e.cost
    args = (lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q), g.get_eom(e.wind), g._state_symbols, q.num_nodes, h)
    with pytest.raises(ValueError, match='lowered for the largest step'):
        odc.Problem(*args, known_parameter_map={}, instance_constraints=q._instance_constraints, bounds=bounds, keep_out=[ko])
    with pytest.raises(NotImplementedError, match='MovingKeepOut in keep_out together with a variable duration'):
        odc.Problem(*args, known_parameter_map={}, instance_constraints=q._instance_constraints, bounds={**bounds, h: (0.05, 0.2)},
                    keep_out=[ou.MovingKeepOut.linear((90.0, 0.0), (0.0, 5.0), 4.0)])
    pr = odc.Problem(*args, known_parameter_map={}, instance_constraints=q._instance_constraints, bounds={**bounds, h: (0.05, 0.2)}, keep_out=[ko], fence=gf)
    assert pr.keep_rows[0, 2] == K.lowered_radius(5.0, 1.0, e.v_constraint[1], 0.2)
