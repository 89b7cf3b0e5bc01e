"""CPU: the statement of the collocation solve with hard keep-out discs (tests/nlp_keepout_ref.py) against oracle.nlp.solve (no discs: bit
for bit), its own derivatives, bisection of the ratio test, the lowering formula, the SLSQP arbiter, the cases of the GPU step
comparison, and the host refusals.

Measured (the statement against tests/golden/nlp_keepout_slsqp.npz, 6 cases of 5, 9 and 17 nodes, one disc 0.3 R off the axis / the same
and a second one that closes the near side; SLSQP stops at ftol 1e-13, the statement at opt_tol 1e-7): relative differences of the cost
  1.1e-09, 7.1e-10, 2.6e-10, 1.5e-09, 2.5e-09, 8.6e-10
so the tolerance is 10 x the largest: 2.6e-8.  (Node values are not compared: they are not unique in the flat directions of the
objective)
"""
import os
import re

import numpy as np
import pytest

import nlp_keepout_ref as K
import nlp_steps_ref as S
from oracle import nlp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'nlp_keepout_slsqp.npz')
SLSQP_COST_RTOL = 2.6e-8         # 10 x the largest relative difference the statement shows over the golden's cases (module docstring)

def test_no_discs_is_oracle_nlp_bit_for_bit():
    for N, tag in ((5, 'disc1'), (17, 'disc0'), (17, 'windbox'), (41, 'bankmax')):
        case, r = S.plain_case(N, tag, 0)
        pb = nlp.problem_from_row(r, N, S.H)
        Wa, ia = nlp.solve(pb, case.W0[0])
        for discs in (np.zeros((0, 3)), np.zeros((3, 3))):           # none, and absent rows (R = 0)
            Wb, ib = K.solve(K.Plain(pb), case.W0[0], discs)
            assert np.array_equal(Wa, Wb) and ia['inner'] == ib['inner'] and ia['status'] == ib['status'] and ia['cost'] == ib['cost']
            assert np.array_equal(ia['mult'], ib['mult']) and ia['path'] == ib['path'] and not ib['zk'].any()


def test_barrier_gradient_and_block_match_central_differences():
    """rhs (with mub / g) is minus the gradient of - mub sum log g; with z = mub / g the 2x2 block (doubled: half convention) is its
    Hessian; the stationarity term is rhs with z for mub / g.  Step 1e-5 on values of order 1 .. 10: first differences to 1e-8, second
    differences to eps / e^2 ~ 1e-6 relative; tolerances 1e-6 and 1e-4 of the largest entry."""
    rng = np.random.default_rng(3)
    N = 9
    W = rng.uniform(-5, 5, (N, 5))
    act = np.array([(0.5, -0.3, 1.2), (8.0, 7.0, 2.0)])
    for cx, cy, R in act:                        # (no node closer than 1.5 R: at g -> 0 the fourth derivative outgrows the step)
        d = W[:, :2] - (cx, cy); dn = np.hypot(*d.T)
        W[:, :2] = np.where((dn < 1.5 * R)[:, None], (cx, cy) + d * (1.5 * R / dn)[:, None], W[:, :2])
    mub = 0.03
    gk = K.g_values(W[1:-1], act)[0]
    assert (gk > 0).all()
    rhs, st, blk = K.barrier_terms(W, act, mub / gk, mub)
    e = 1e-5
    f = lambda W: K.barrier_value(W, act, mub)          # noqa: E731
    grad = np.zeros((N, 2)); hess = np.zeros((N, 2, 2))
    for i in range(N):
        for c in range(2):
            Wp = W.copy(); Wp[i, c] += e; Wm = W.copy(); Wm[i, c] -= e
            grad[i, c] = (f(Wp) - f(Wm)) / (2 * e)
            for d in range(2):
                e2 = 1e-4
                Wpp = W.copy(); Wpp[i, c] += e2; Wpp[i, d] += e2; Wpm = W.copy(); Wpm[i, c] += e2; Wpm[i, d] -= e2
                Wmp = W.copy(); Wmp[i, c] -= e2; Wmp[i, d] += e2; Wmm = W.copy(); Wmm[i, c] -= e2; Wmm[i, d] -= e2
                hess[i, c, d] = (f(Wpp) - f(Wpm) - f(Wmp) + f(Wmm)) / (4 * e2 * e2)
    assert not grad[0].any() and not grad[-1].any() and not rhs[0].any()          # the end nodes carry no disc term
    assert np.abs(-rhs - grad).max() <= 1e-6 * np.abs(grad).max()
    assert np.abs(2 * blk - hess).max() <= 1e-4 * np.abs(hess).max(), (np.abs(2 * blk - hess).max(), np.abs(hess).max())
    assert np.allclose(st, -rhs, rtol=1e-13, atol=0)                              # z = mub / g: on the central path the two agree
    # the block keeps the constraint's own curvature: trace = 2 (z / g) |d|^2 - 2 z per disc, and it is indefinite near a disc
    assert (np.linalg.eigvalsh(blk[1:-1]).min(axis=1) < 0).any()


def test_ratio_test_against_bisection():
    """The closed form against bisection of  g(a) = g + 2 a d.s + a^2 |s|^2 - (1 - tau) g  for the FIRST zero on [0, 1] (scanned on a
    grid of 4096 points, then bisected), on random (g, d, s): steps that miss, that end inside, and that cross the disc and come out
    again (g(1) > 0 with a zero before it).  A linearised test errs in both directions: both are counted."""
    rng = np.random.default_rng(11)
    tau = 0.99
    n_cross = n_lin_long = n_lin_short = 0
    for _ in range(400):
        R = rng.uniform(0.5, 3.0)
        ang = rng.uniform(0, 2 * np.pi)
        d = R * rng.uniform(1.001, 2.5) * np.array([np.cos(ang), np.sin(ang)])
        s = rng.uniform(0.1, 8.0) * np.array([np.cos(ang + np.pi + rng.normal(0, 0.6)), np.sin(ang + np.pi + rng.normal(0, 0.6))])
        g = d @ d - R * R
        q = lambda a: g + 2 * a * (d @ s) + a * a * (s @ s) - (1 - tau) * g          # noqa: E731
        a_cf = float(K.ratio_disc(g, d @ s, s @ s, tau))
        grid = np.linspace(0.0, 1.0, 4097)
        neg = np.flatnonzero(q(grid) < 0)
        if len(neg) == 0:
            assert a_cf >= 1.0 - 1e-3, (a_cf,)          # (a double root between two grid points: the closed form may see it)
            continue
        lo, hi = grid[neg[0] - 1], grid[neg[0]]
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if q(mid) >= 0 else (lo, mid)
        assert abs(a_cf - lo) <= 1e-12 * max(1.0, lo), (a_cf, lo)
        n_cross += q(1.0) > 0
        a_lin = tau * g / (-2 * (d @ s)) if d @ s < 0 else np.inf
        n_lin_long += a_lin > a_cf * (1 + 1e-9); n_lin_short += a_lin < a_cf * (1 - 1e-9)
    print(f'{n_cross} steps cross the disc and come out again; the linearised test is longer {n_lin_long} times, shorter {n_lin_short} times')
    assert n_cross >= 20 and n_lin_short >= 20
    assert n_lin_long == 0          # (the quadratic term is positive: the linear test is never longer -- it is wrong by being short,
    #                                  and by seeing a limit where the step passes the disc by: counted next)
    miss = 0
    for _ in range(200):
        d = np.array([2.0, 0.0]); R = 1.0; g = d @ d - R * R
        s = np.array([-rng.uniform(0.5, 4.0), rng.choice([-1, 1]) * rng.uniform(1.5, 4.0)])
        if np.isinf(K.ratio_disc(g, d @ s, s @ s, tau)):
            miss += (tau * g / (-2 * (d @ s))) < 1.0
    assert miss >= 20               # the linear test cuts steps that never reach the disc


def test_lowering_keeps_the_margin_on_the_polyline():
    """Every point of a polyline whose nodes satisfy g >= 0 for R = lowered_radius(r, margin, v_max, h), at spacing <= v_max h, keeps
    `margin` from the disc: checked on node pairs ON the circle at the largest spacing (the worst case, where the bound is attained) and
    on random polylines outside it."""
    import d2d.opty_utils as ou
    rng = np.random.default_rng(5)
    for _ in range(200):
        r, margin, v_max, h = rng.uniform(0.5, 20), rng.uniform(0, 3), rng.uniform(9, 20), rng.uniform(0.02, 0.3)
        ko = ou.KeepOut((1.0, -2.0), r, margin)
        cx, cy, R = ko.lowered(v_max, h)
        assert R == K.lowered_radius(r, margin, v_max, h)
        half = np.arcsin(min(1.0, 0.5 * v_max * h / R))
        th = rng.uniform(0, 2 * np.pi)
        xy = np.array([(cx + R * np.cos(th - half), cy + R * np.sin(th - half)), (cx + R * np.cos(th + half), cy + R * np.sin(th + half))])
        cl = ou.keep_out_clearance([ko], xy[:, 0], xy[:, 1])[0]
        assert cl >= margin - 1e-9 * R and cl <= margin + 1e-9 * R           # attained
        assert abs(cl - K.polyline_clearance(xy, ko.c, r)) <= 1e-12 * R
        # a random walk of steps <= v_max h whose nodes are pushed out of the circle R
        p = np.array([cx - 1.5 * R, cy + rng.uniform(-R, R)]); pts = []
        for _k in range(80):
            stp = rng.uniform(0.2, 1.0) * v_max * h
            q = p + stp * np.array([np.cos(rng.normal(0, 0.5)), np.sin(rng.normal(0, 0.5))])
            dq = q - (cx, cy)
            if dq @ dq < R * R:
                q = np.array((cx, cy)) + dq * (R / np.sqrt(dq @ dq)) * (1 + 1e-12)
            if np.hypot(*(q - p)) <= v_max * h:
                p = q; pts.append(p)
        pts = np.array(pts)
        assert ou.keep_out_clearance([ko], pts[:, 0], pts[:, 1])[0] >= margin - 1e-9 * R


def test_start_rule_and_refusals():
    pb, r, W0, L = K.leg_problem(17, 0)
    mid = 0.5 * (pb.p0[:2] + pb.p1[:2])
    R = 0.1 * L
    # radial push; the degenerate direction goes along the left normal of the leg
    W = W0.copy(); W[8, :2] = mid
    Ws = K.start(pb, W, np.array([(mid[0], mid[1], R)]))
    leg = pb.p1[:2] - pb.p0[:2]; nrm = np.array([-leg[1], leg[0]]) / np.hypot(*leg)
    assert np.allclose(Ws[8, :2], mid + 1.01 * R * nrm, rtol=0, atol=1e-12)
    assert (K.g_values(Ws[1:-1], np.array([(mid[0], mid[1], R)]))[0] > 0).all()
    assert np.array_equal(Ws[[0, -1]], W[[0, -1]]) and np.array_equal(Ws[:, 2:], W[:, 2:])
    # two passes undo a push out of one disc into its neighbour
    # (the node starts outside the first disc and inside the second, whose push puts it into the first: only the second pass sees that)
    two = np.array([(mid[0], mid[1], R), (mid[0] + 1.032 * R, mid[1] + 0.728 * R, 1.183 * R)])
    W = W0.copy(); W[1:-1, :2] = mid + (0.0, 5.0 * R); W[8, :2] = mid + (0.959 * R, 0.461 * R)
    g0 = K.g_values(W[8:9], two)[0][:, 0]
    assert g0[0] > 0.0201 * R * R and g0[1] < 0
    Ws = K.start(pb, W, two)
    assert (K.g_values(Ws[1:-1], two)[0] > 0).all() and not np.array_equal(Ws[8, :2], W[8, :2])
    # ... and discs that overlap along the push direction hand the node back and forth: refused, not solved from inside a disc
    pp = np.array([(mid[0], mid[1], R), (mid[0], mid[1] + 1.6 * R, 0.7 * R)])
    W = W0.copy(); W[1:-1, :2] = mid + (0.0, 5.0 * R); W[8, :2] = mid + (0.0, 0.5 * R)
    assert K.refused(pb, pp, K.start(pb, W, pp)) and K.solve(K.Plain(pb), W, pp)[1]['status'] == K.ST_NONFINITE
    prob = K.Plain(pb)
    for bad in (np.array([(mid[0], mid[1], np.nan)]), np.array([(np.inf, mid[1], R)]), np.array([(mid[0], mid[1], 0.0), (pb.p0[0], pb.p0[1] + 0.5, 1.0)]),
                np.array([(pb.p1[0] + 1.0, pb.p1[1], 1.0)])):
        Wr, info = K.solve(prob, W0, bad)
        assert info['status'] == K.ST_NONFINITE and np.isnan(info['cost']) and np.isnan(info['feas']) and np.array_equal(Wr, W0) and info['inner'] == 0
    # discs that cover the y box: no free node has a place
    pbb, _, W0b, Lb = K.leg_problem(17, 0, y_box=True)
    cover = np.array([(0.5 * Lb, 0.0, 0.3 * Lb)])
    assert K.solve(K.Plain(pbb), W0b, cover)[1]['status'] == K.ST_NONFINITE


def golden_cases():
    g = np.load(GOLDEN)
    for k in range(int(g['n_cases'])):
        N = int(g[f'c{k}_N'])
        yield k, nlp.problem_from_row(g[f'c{k}_row'], N, K.H0), g[f'c{k}_row'], g[f'c{k}_W0'], g[f'c{k}_discs'], float(g[f'c{k}_cost'])


def test_statement_vs_slsqp_golden():
    worst = 0.0
    for k, pb, _, W0, discs, cost in golden_cases():
        W, info = K.solve(K.Plain(pb), W0, discs)
        dc = abs(info['cost'] - cost) / cost
        worst = max(worst, dc)
        gk = K.g_values(W[1:-1], discs)[0]
        print(f'case {k} (N {pb.N}, {len(discs)} discs): status {info["status"]}, {info["inner"]} steps, cost off by {dc:.2e} relative, min g / R^2 {(gk / discs[:, 2:3] ** 2).min():.1e}')
        assert info['status'] == 1 and info['feas'] <= 1e-9 and (gk > 0).all()
        assert (gk / discs[:, 2:3] ** 2).min() < 1e-6           # the disc binds: the case tests the constraint
        assert dc <= SLSQP_COST_RTOL
    print(f'largest: {worst:.2e}')


def test_full_solves_hold_the_margin_where_the_soft_cost_cuts():
    for N in K.FULL_N:
        for prob, r, W0, discs, (c, ru, margin) in K.full_launch(N):
            W, info = K.solve(prob, W0, discs)
            act = discs[discs[:, 2] > 0]
            gk = K.g_values(W[1:-1], act)[0]
            zk = info['zk'][:len(act), 1:-1]
            k = np.unravel_index(np.argmin(gk / act[:, 2:3] ** 2), gk.shape)
            assert info['status'] == 1 and info['feas'] <= 1e-9 and (gk > 0).all()
            assert gk[k] / act[k[0], 2] ** 2 < 1e-6 and zk[k] > 1e-3 * zk.max()
            assert np.abs(zk * gk - nlp.MUB_MIN).max() <= 1e-7
            assert K.polyline_clearance(W[:, :2], c, ru) >= margin
            Ws, si = nlp.solve(nlp.problem_from_row(r, N, K.H0), W0)
            assert si['status'] == 1 and K.polyline_clearance(Ws[:, :2], c, ru) < 0.0


@pytest.mark.parametrize('N', K.STEP_N)
def test_step_cases_are_determined(N):
    """Every case of the GPU step comparison, on the statement alone (nlp_steps_ref.check): its tolerance is at most 1e-8 and the
    perturbed starts take the same path after every budget; budgets with outer_max = 1 end at 'max iterations' with every step
    accepted and moving W by 1e6 tolerances.  At 3 and 5 nodes the first inner problem is solved within 8 steps, so there the budget
    (8, 1) is held to the first two checks only.  The cases that are to bind do so inside the budgets: a dual of at least 1."""
    for tag, (case, r, discs, prob) in K.steps_launch(N).items():
        zmax = 0.0
        for budget in S.BUDGETS:
            bad = S.check(case, budget)
            if N <= 5 and budget == (8, 1):
                bad = [b for b in bad if b.startswith('tol') or b.startswith('the perturbed')]
            assert not bad, (case.cid, budget, bad)
            zmax = max(zmax, float(S.measure(case, budget)['info']['raw']['zk'].max()))
        if tag != 'many':
            assert zmax >= 1.0, (case.cid, zmax)
        else:
            assert (discs[[2, 5], 2] == 0.0).all() and (discs[:, 2] > 0).sum() == K.MAX_KEEP - 2


# ---- host layers --------------------------------------------------------------------------------------------------------------------
def _exp14(**attrs):
    import d2d.optyplan_scenarios as sc
    return type('exp_14_k', (sc.exp_14,), attrs)


def _disc_across(e):
    """A disc of 5 m, margin 1 m, across exp_14's free plan, which passes (1.88, -3.54) at its middle node heading 0.588 rad (oracle.nlp
    from the 'tri' guess): the centre is 1.4 m off that track, so the free plan goes 3.6 m deep into the disc."""
    import d2d.opty_utils as ou
    assert e.__name__.startswith('exp_14')
    return ou.KeepOut((2.88, -4.54), 5.0, margin=1.0)


def test_keep_out_is_validated_and_refused_by_name():
    import d2d.opty_utils as ou
    import d2dhip
    import full_sim
    import multi_opt_planner as mop
    import single_opt_planner as sop
    for bad in (dict(c=(0, 0), r=0.0), dict(c=(0, 0), r=-1.0), dict(c=(0, np.nan), r=1.0), dict(c=(0, 0), r=1.0, margin=-0.1), dict(c=(0, 0), r=np.inf)):
        with pytest.raises(ValueError, match='KeepOut'):
            ou.KeepOut(**bad)
    import d2d.optyplan_scenarios as sc
    ko = _disc_across(sc.exp_14)
    with pytest.raises(NotImplementedError, match="backend='fit'"):
        sop.Planner(_exp14(keep_out=[ko]), backend='fit')
    with pytest.raises(NotImplementedError, match='moving obstacles'):
        sop.Planner(_exp14(keep_out=[ko], moving_obstacles=[ou.MovingObstacle.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), backend='nlp')
    with pytest.raises(NotImplementedError, match='waypoints'):
        sop.Planner(_exp14(keep_out=[ko], waypoints=[ou.Waypoint(sc.exp_14.t0 + 1.0, x=1.0)]), backend='nlp')
    with pytest.raises(NotImplementedError, match='t1_free'):
        sop.Planner(_exp14(keep_out=[ko], t1_free=(sc.exp_14.t1 - 1.0, sc.exp_14.t1 + 1.0)), backend='nlp')
    with pytest.raises(NotImplementedError, match=f'at most {d2dhip.MAX_KEEP}'):
        sop.Planner(_exp14(keep_out=[ko] * (d2dhip.MAX_KEEP + 1)), backend='nlp')
    import d2d.multioptyplan_scenarios as msc
    ms = next(getattr(msc, n) for n in dir(msc) if n.startswith('exp_') and hasattr(getattr(msc, n), 'p0s'))
    with pytest.raises(NotImplementedError, match='keep_out'):
        mop.Planner(type('m_k', (ms,), dict(keep_out=[ko])), backend='nlp')
    # 'auto' goes straight to the collocation backend, and the lowering is the formula
    import opty.direct_collocation as odc
    p = sop.Planner(_exp14(keep_out=[ko]), backend='auto')
    assert isinstance(p.prob, odc.Problem) and p.prob.keep_out == [ko]
    assert np.array_equal(p.prob.keep_rows, [ko.lowered(sc.exp_14.v_constraint[1], p.time_step)])
    assert p.prob.keep_rows[0, 2] == K.lowered_radius(5.0, 1.0, sc.exp_14.v_constraint[1], p.time_step)
    assert isinstance(sop.Planner(_exp14()).prob, sop._FitProblem) and not sop.Planner(_exp14()).keep_out         # without it: as before
    # plan_batch and nlp_plan: each pair by name, before any device is touched
    rows, W0 = np.zeros((2, d2dhip.SCEN_STRIDE)), np.zeros((2, 5, 41))
    kk = np.zeros((2, 1, 3))
    for kw, name in ((dict(n_ac=2), 'n_ac > 1'), (dict(moving=[ou.MovingObstacle.linear((0, 0), (1, 0), 1.0)]), 'moving'), (dict(via=[[], []]), 'via'),
                     (dict(free_time=(0.05, 0.2)), 'free_time')):
        with pytest.raises(NotImplementedError, match=name):
            full_sim.plan_batch(rows, 41, 4.0, 1.0 / 41, backend='nlp', W0=W0, h=0.1, keep_out=kk, **kw)
    with pytest.raises(NotImplementedError, match='polynomial fit'):
        full_sim.plan_batch(rows, 41, 4.0, 1.0 / 41, backend='fit', keep_out=kk)
    for kw, name in ((dict(n_ac=2), 'n_ac'), (dict(free_rows=kk), 'free_rows'), (dict(via=kk), 'via'), (dict(knots=kk), 'knots')):
        with pytest.raises(NotImplementedError, match=f'keep together with {name}'):
            d2dhip.nlp_plan(None, None, None, 0.1, keep=kk, **kw)


def test_mission_chain_host_objective_and_several_aircraft_refuse_by_name():
    import d2d.optyplan_scenarios as sc
    import d2d.opty_utils as ou
    import full_sim
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    ko = _disc_across(sc.exp_14)
    # the mission chain: refused on entry, before a context is made or anything is launched (every other argument is a place holder)
    with pytest.raises(NotImplementedError, match='mission chain has no hard keep-out discs'):
        full_sim.full_sim_phases_batch(None, None, None, 2, None, type('m', (), dict(keep_out=[ko])), None, 10.0)

    class Odd:                                   # a cost plug-in no kernel knows: the host objective
        def cost(self, free, planner):
            return float(np.sum(free ** 2))

        def cost_grad(self, free, planner):
            return 2.0 * free
    with pytest.raises(NotImplementedError, match='keep_out together with a host objective'):
        sop.Planner(_exp14(keep_out=[ko], cost=Odd()), backend='nlp')
    q = sop.Planner(_exp14(), backend='nlp')
    e, g = _exp14(), q.aircraft
    odd = Odd()
    with pytest.raises(NotImplementedError, match='keep_out together with the host objective'):
        odc.Problem(lambda f: odd.cost(f, q), lambda f: odd.cost_grad(f, q), g.get_eom(e.wind), g._state_symbols, q.num_nodes, q.time_step,
                    known_parameter_map={}, instance_constraints=q._instance_constraints, bounds=q._bounds, keep_out=[ko])
    cost = e.cost
    g2 = [ou.Aircraft(id='_0'), ou.Aircraft(id='_1')]
    ic = tuple(s(t) - 0.0 for a in g2 for s in (a._sx, a._sy, a._spsi) for t in (0.0, 3.0))
    b2 = {a._sphi(a._st): e.phi_constraint for a in g2}; b2.update({a._sv(a._st): e.v_constraint for a in g2})
    with pytest.raises(NotImplementedError, match='keep_out together with more than one aircraft'):
        odc.Problem(lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q), ou.Eom((0.0, 0.0), ids=('_0', '_1')),
                    g2[0]._state_symbols + g2[1]._state_symbols, 31, 0.1, instance_constraints=ic, bounds=b2, keep_out=[ko])


def test_header_version_and_binding():
    import d2dhip
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 121
    assert 'd2d_nlp_solve_keepout' in hdr and 'd2d_keep_out' in hdr
    assert int(re.search(r'#define D2D_MAX_KEEP (\d+)', hdr).group(1)) == d2dhip.MAX_KEEP == K.MAX_KEEP
    assert 'd2d_nlp_solve_keepout' in d2dhip.EXPORTS
