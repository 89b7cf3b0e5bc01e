"""CPU: the statement of the collocation solve with hard keep-out discs that move (tests/nlp_keepout_moving_ref.py) against the static
statement (tracks that stand still: bit for bit) and oracle.nlp.solve (no discs), its own derivatives with per-node centres, the
relative-chord bound, the lowering formula, the cases of the GPU step comparison, the new routes of d2dhip.nlp_plan against a fake
context and every new refusal by name -- and the sentence of the change: on scenario 1 of tests/test_gpu_deconflict.py at margin 0 the
soft loop ends BELOW d_sep and the hard one at or above it.
"""
import os
import re

import numpy as np
import pytest

import nlp_keepout_moving_ref as KM
import nlp_keepout_ref as K
import nlp_steps_ref as S
from oracle import nlp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'nlp_keepout_moving_slsqp.npz')
SLSQP_COST_RTOL = 2.2e-8         # 10 x the largest relative difference measured when the golden file was made (its generator's docstring)


def golden_cases():
    """-> (k, oracle Problem, row, W0, [track], t_start, SLSQP's cost) of every case of the golden file, the problem rebuilt from the
    stored row and track (and held equal to nlp_keepout_moving_ref.arbiter_problem's)."""
    g = np.load(GOLDEN)
    for k in range(int(g['n_cases'])):
        N, kind = int(g[f'c{k}_N']), str(g[f'c{k}_kind'])
        pb, row, W0, trs = KM.arbiter_problem(N, kind)
        assert np.array_equal(row, g[f'c{k}_row']) and np.array_equal(W0, g[f'c{k}_W0']) and np.array_equal(trs[0].padded(2), g[f'c{k}_knots'])
        assert trs[0].r == float(g[f'c{k}_R']) and KM.ARB_T_START == float(g[f'c{k}_t_start'])
        yield k, pb, row, W0, trs, KM.ARB_T_START, float(g[f'c{k}_cost'])


def test_statement_vs_slsqp_golden():
    """The independent arbiter: scipy SLSQP with the node inequalities as true constraints (5, 9, 17 nodes; a crossing and an overtaking
    disc).  The statement ends converged, on the disc, at SLSQP's cost."""
    worst, n = 0.0, 0
    for k, pb, row, W0, trs, t0, cost in golden_cases():
        W, info = KM.solve_moving(pb, W0, trs, t0)
        ctr, R = KM.centres(trs, t0, pb.N, pb.h)
        gk = KM.g_values(W[1:-1], ctr[:, 1:-1], R)[0]
        dc = abs(info['cost'] - cost) / cost
        worst, n = max(worst, dc), n + 1
        print(f'case {k} (N {pb.N}): status {info["status"]}, cost off by {dc:.2e} relative, min g / R^2 {gk.min() / R[0] ** 2:.1e}')
        assert info['status'] == 1 and gk.min() >= 0.0 and gk.min() / R[0] ** 2 < 1e-6          # converged, outside, and the disc binds
        assert dc <= SLSQP_COST_RTOL
    print(f'largest: {worst:.2e}')
    assert n == 6
    # the discs matter: without them the plan of the 17-node cases is cheaper and cuts the disc
    for k, pb, row, W0, trs, t0, cost in golden_cases():
        if pb.N == 17:
            Wf, i0 = nlp.solve(pb, W0)
            ctr, R = KM.centres(trs, t0, pb.N, pb.h)
            assert i0['cost'] < cost * (1 - 1e-6) and KM.g_values(Wf[1:-1], ctr[:, 1:-1], R)[0].min() < 0.0


def test_tracks_that_stand_still_are_the_static_statement_bit_for_bit():
    for N, tag in ((5, 'bind'), (17, 'two'), (17, 'many'), (17, 'shear')):
        case, r, discs, prob = K.steps_launch(N)[tag]
        W0 = case.W0[0][:N]
        Wa, ia = K.solve(prob, W0, discs)
        Wb, ib = KM.solve(prob, W0, *KM.constant_centres(discs, N))
        assert ia['status'] != KM.ST_NONFINITE and ia['inner'] > 5
        assert np.array_equal(Wa, Wb) and ia['inner'] == ib['inner'] and ia['status'] == ib['status'] and ia['cost'] == ib['cost']
        assert np.array_equal(ia['mult'], ib['mult']) and ia['path'] == ib['path'] and np.array_equal(ia['zk'], ib['zk'])
    prob, r, W0, discs, _ = K.full_launch(41)[1]
    Wa, ia = K.solve(prob, W0, discs)
    Wb, ib = KM.solve(prob, W0, *KM.constant_centres(discs, 41))
    assert ia['status'] == 1 and np.array_equal(Wa, Wb) and ia['path'] == ib['path'] and np.array_equal(ia['zk'], ib['zk'])
    # a refused static problem is refused alike
    inside = discs.copy(); inside[1] = (prob.pb.p1[0] + 0.5, prob.pb.p1[1], 1.0)
    assert K.solve(prob, W0, inside)[1]['status'] == KM.solve(prob, W0, *KM.constant_centres(inside, 41))[1]['status'] == KM.ST_NONFINITE


def test_no_discs_is_oracle_nlp_bit_for_bit():
    for N, tag in ((5, 'disc1'), (17, 'windbox')):
        case, r = S.plain_case(N, tag, 0)
        pb = nlp.problem_from_row(r, N, S.H)
        Wa, ia = nlp.solve(pb, case.W0[0])
        for ctr, R in ((np.zeros((0, N, 2)), np.zeros(0)), (np.ones((3, N, 2)), np.array([0.0, -1.0, 0.0]))):      # none, and absent slots
            Wb, ib = KM.solve(KM.Plain(pb), case.W0[0], ctr, R)
            assert np.array_equal(Wa, Wb) and ia['inner'] == ib['inner'] and ia['status'] == ib['status'] and ia['cost'] == ib['cost']
            assert np.array_equal(ia['mult'], ib['mult']) and ia['path'] == ib['path'] and not ib['zk'].any()


def test_barrier_gradient_and_block_match_central_differences_with_per_node_centres():
    """tests/test_nlp_keepout_cpu.py's check with every node's own centre: steps 1e-5 / 1e-4 on values of order 1 .. 10, tolerances
    1e-6 and 1e-4 of the largest entry.  The centres are data: no term for their motion appears."""
    rng = np.random.default_rng(5)
    N = 9
    W = rng.uniform(-5, 5, (N, 5))
    R = np.array([1.2, 2.0])
    ctr = np.stack([np.array([0.5, -0.3]) + np.outer(np.arange(N), (0.4, -0.2)), np.array([8.0, 7.0]) + np.outer(np.arange(N), (-0.9, -0.6))])
    for m in range(2):
        d = W[:, :2] - ctr[m]; dn = np.hypot(*d.T)
        W[:, :2] = np.where((dn < 1.5 * R[m])[:, None], ctr[m] + d * (1.5 * R[m] / dn)[:, None], W[:, :2])
    mub = 0.03
    gk = KM.g_values(W[1:-1], ctr[:, 1:-1], R)[0]
    assert (gk > 0).all()
    rhs, st, blk = KM.barrier_terms(W, ctr, R, mub / gk, mub)
    f = lambda W: KM.barrier_value(W, ctr, R, mub)          # noqa: E731
    grad = np.zeros((N, 2)); hess = np.zeros((N, 2, 2))
    e, e2 = 1e-5, 1e-4
    for i in range(N):
        for c in range(2):
            Wp = W.copy(); Wp[i, c] += e; Wm = W.copy(); Wm[i, c] -= e
            grad[i, c] = (f(Wp) - f(Wm)) / (2 * e)
            for d in range(2):
                Wpp = W.copy(); Wpp[i, c] += e2; Wpp[i, d] += e2; Wpm = W.copy(); Wpm[i, c] += e2; Wpm[i, d] -= e2
                Wmp = W.copy(); Wmp[i, c] -= e2; Wmp[i, d] += e2; Wmm = W.copy(); Wmm[i, c] -= e2; Wmm[i, d] -= e2
                hess[i, c, d] = (f(Wpp) - f(Wpm) - f(Wmp) + f(Wmm)) / (4 * e2 * e2)
    assert not grad[0].any() and not grad[-1].any() and not rhs[0].any()
    assert np.abs(-rhs - grad).max() <= 1e-6 * np.abs(grad).max()
    assert np.abs(2 * blk - hess).max() <= 1e-4 * np.abs(hess).max()
    assert np.allclose(st, -rhs, rtol=1e-13, atol=0)
    # the static terms with one centre for all nodes are NOT these: the per-node centre is read
    assert np.abs(K.barrier_terms(W, np.array([(0.5, -0.3, 1.2), (8.0, 7.0, 2.0)]), mub / gk, mub)[0] - rhs).max() > 1e-3


def test_the_relative_chord_bound():
    """400 random segments d0 -> d1 of the RELATIVE position with |d0|, |d1| >= R and |d1 - d0| <= s: the smallest distance from the
    origin along the segment is >= sqrt(R^2 - (s / 2)^2), attained by the chord with both ends on the circle at spacing s."""
    rng = np.random.default_rng(11)
    worst = np.inf
    for k in range(400):
        R = rng.uniform(0.5, 6.0); s = rng.uniform(0.05, 1.9) * R
        a0 = rng.uniform(0, 2 * np.pi)
        d0 = R * (1.0 + (rng.uniform(0, 0.3) if k % 3 else 0.0)) * np.array([np.cos(a0), np.sin(a0)])
        for _ in range(200):                      # a second end within s of the first and outside the circle
            a1 = rng.uniform(0, 2 * np.pi); d1 = d0 + s * np.sqrt(rng.uniform(0, 1)) * np.array([np.cos(a1), np.sin(a1)])
            if np.hypot(*d1) >= R:
                break
        else:
            d1 = d0
        if k % 5 == 0:                            # the worst case: both ends ON the circle, exactly s apart
            half = np.arcsin(min(0.5 * s / R, 1.0))
            d0 = R * np.array([np.cos(a0 - half), np.sin(a0 - half)]); d1 = R * np.array([np.cos(a0 + half), np.sin(a0 + half)])
        ab = d1 - d0
        t = np.clip(-np.dot(d0, ab) / max(np.dot(ab, ab), 1e-300), 0.0, 1.0)
        dmin = float(np.hypot(*(d0 + t * ab)))
        bound = KM.chord_bound(R, s)
        worst = min(worst, (dmin - bound) / R)
        assert dmin >= bound - 1e-12 * R, (k, dmin, bound)
    print(f'smallest (distance - bound) / R: {worst:.2e}')
    assert worst <= 1e-12                          # the bound is attained
    # deconflict_hard's radius: two aircraft that each move at most step_max between two rows
    assert abs(KM.chord_bound(KM.hard_radius(4.0, 0.5, 2.0), 2 * 2.0) - 4.5) <= 1e-12


def test_lowering():
    import d2d.opty_utils as ou
    import d2dhip
    ko = ou.MovingKeepOut((1.0, 3.0, 4.0), ((0.0, 0.0), (6.0, 8.0), (6.0, 9.0)), 2.0, margin=0.5)
    assert ko.v_c == 5.0                           # the fastest knot segment: 10 m in 2 s (then 1 m in 1 s)
    R = ko.lowered(14.0, 0.1)
    assert R == float(np.sqrt(2.5 ** 2 + (0.5 * 19.0 * 0.1) ** 2))
    assert abs(KM.chord_bound(R, (14.0 + 5.0) * 0.1) - 2.5) <= 1e-12
    st = ou.KeepOut((3.0, -1.0), 2.0, margin=0.25)
    knots, disc = ou.lower_keep_moving([ko, st], 14.0, 0.1, 4)
    assert knots.shape == (2, 4, 3) and disc.shape == (2, 2) and (disc[:, 1] == 1).all()
    assert disc[0, 0] == R and disc[1, 0] == st.lowered(14.0, 0.1)[2]
    assert np.array_equal(knots[0, :3, 0], ko.t) and np.array_equal(knots[0, :3, 1:], ko.xy) and (np.diff(knots[:, :, 0], axis=1) > 0).all()
    assert (knots[1, :, 1:] == (3.0, -1.0)).all()                      # a static disc: a track that stands still
    assert np.array_equal(ou.track_at(knots[0, :, 0], knots[0, :, 1:], np.array([0.0, 2.0, 9.0])), ko.at(np.array([0.0, 2.0, 9.0])))
    for bad in (dict(r=0.0), dict(r=np.nan), dict(margin=-1.0)):
        with pytest.raises(ValueError, match='MovingKeepOut'):
            ou.MovingKeepOut((0.0, 1.0), ((0.0, 0.0), (1.0, 1.0)), **{'r': 1.0, **bad})
    with pytest.raises(ValueError, match='increase strictly'):
        ou.MovingKeepOut((0.0, 0.0), ((0.0, 0.0), (1.0, 1.0)), 1.0)
    with pytest.raises(NotImplementedError, match='at most'):
        ou.lower_keep_moving([ko] * (d2dhip.MAX_MOV + 1), 14.0, 0.1)
    # the continuous clearance: an aircraft that flies +x at 10 m/s past a disc that comes down the y axis
    t = np.arange(11) * 0.1
    mk = ou.MovingKeepOut.linear((0.5, 1.0), (0.0, -1.0), 0.25, t0=0.0, t1=1.0)
    cl = ou.moving_keep_clearance([mk], t, 10.0 * t - 0.2, np.zeros(11))[0]
    rel0, rv = np.array([-0.7, -1.0]), np.array([10.0, 1.0])           # relative position p - c at t = 0 and its velocity
    ts = -np.dot(rel0, rv) / np.dot(rv, rv)
    assert 0.0 < ts < 1.0 and abs(cl - (np.hypot(*(rel0 + ts * rv)) - 0.25)) <= 1e-12
    assert cl < min(np.hypot(10.0 * t - 0.2 - 0.5, -(1.0 - t))) - 0.25   # closer between two nodes than at any node


class _Stub:
    """A context that records which entry nlp_plan calls, as tests/test_nlp_dispatch_cpu.py does."""

    def __getattr__(self, name):
        if not name.startswith('nlp_solve'):
            raise AttributeError(name)
        return lambda scen, W, h, *more, **kw: dict(entry_called=name, args=(scen, W, h), kw=kw)


def test_nlp_plan_routes_and_refusals():
    import d2dhip
    out = d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, hard_knots='K', hard_disc='D', t_start='T', bounds='B')
    assert out['entry'] == out['entry_called'] == 'nlp_solve_keepout_moving' and out['args'] == ('S', 'W', 0.1)
    assert out['kw'] == dict(knots='K', disc='D', field=None, t_start='T', bounds='B')
    out = d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, n_ac=3, hard_knots='K', hard_disc='D', field='F', t_start='T', max_sweeps=5)
    assert out['entry'] == out['entry_called'] == 'nlp_solve_groups_keepout'
    assert out['kw'] == dict(knots='K', disc='D', field='F', t_start='T', n_ac=3, max_sweeps=5)
    for name, kw in (('keep', dict(keep='X')), ('knots', dict(knots='X', disc='Y')), ('disc', dict(disc='Y')), ('via', dict(via='X')),
                     ('free_rows', dict(free_rows='X'))):
        with pytest.raises(NotImplementedError, match=rf'hard_knots together with {name}'):
            d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, hard_knots='K', hard_disc='D', **kw)
    with pytest.raises(ValueError, match='go together'):
        d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, hard_knots='K')
    # every existing route is untouched by the new keywords' defaults
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1)['entry'] == 'nlp_solve'
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, keep='X')['entry'] == 'nlp_solve_keepout'
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, n_ac=2, knots='K', disc='D')['entry'] == 'nlp_solve_groups_moving'


def test_plan_batch_refusals_by_name():
    import d2d.opty_utils as ou
    import full_sim
    mk = [ou.MovingKeepOut.linear((0.0, 5.0), (1.0, 0.0), 2.0)]
    rows = np.zeros((2, 64))
    kw = dict(backend='nlp', W0=np.zeros((2, 5, 9)), h=0.1, hard_moving=mk)
    for name, extra in (('moving', dict(moving=[ou.MovingObstacle.linear((0.0, 0.0), (1.0, 0.0), 2.0)])), ('via', dict(via=[[], []])),
                        ('free_time', dict(free_time=(0.05, 0.2))), ('keep_out', dict(keep_out=[ou.KeepOut((0.0, 0.0), 1.0)])),
                        ('deconflict', dict(deconflict=dict(d_sep=1.0, margin=0.0, d_look=5.0)))):
        with pytest.raises(NotImplementedError, match=rf'hard_moving with {name}'):
            full_sim.plan_batch(rows, 9, 0.8, 1.0, **kw, **extra)
    with pytest.raises(NotImplementedError, match='polynomial fit has no hard moving discs'):
        full_sim.plan_batch(rows, 9, 0.8, 1.0, hard_moving=mk)
    with pytest.raises(ValueError, match='deconflict: needs d_sep'):
        full_sim.plan_batch(rows, 9, 0.8, 1.0, backend='nlp', W0=np.zeros((2, 5, 9)), h=0.1, deconflict=dict(d_sep=1.0, margin=0.0, d_look=5.0, harder=True))


@pytest.mark.parametrize('N', KM.STEP_N)
def test_step_cases_are_determined(N):
    """Every case of the GPU step comparison, on the statement alone (nlp_steps_ref.check), as tests/test_nlp_keepout_cpu.py holds the
    static ones: tolerance at most 1e-8, the same path from the perturbed starts after every budget; budgets with outer_max = 1 end at
    'max iterations' with every step accepted and moving W by 1e6 tolerances (3 and 5 nodes: the budget (8, 1) is held to the first two
    checks only).  Every case binds inside the budgets: a dual of at least 1."""
    for tag, (case, r, trs, prob) in KM.steps_launch(N).items():
        zmax = 0.0
        for budget in S.BUDGETS:
            bad = S.check(case, budget)
            if N <= 5 and budget == (8, 1):
                bad = [b for b in bad if b.startswith('tol') or b.startswith('the perturbed')]
            assert not bad, (case.cid, budget, bad)
            zmax = max(zmax, float(S.measure(case, budget)['info']['raw']['zk'].max()))
        assert zmax >= 1.0, (case.cid, zmax)
        assert sum(t.r > 0 for t in trs) == (6 if tag == 'many' else 1) and len(trs) == KM.MAX_MOV


def test_start_rule_and_refusals_read_the_nodes_own_centre():
    N = 17
    pb, r, W0, L = K.leg_problem(N, 0)
    T = (N - 1) * K.H0
    mid = 0.5 * (pb.p0[:2] + pb.p1[:2]); leg = pb.p1[:2] - pb.p0[:2]; ax = leg / np.hypot(*leg)
    R = 0.1 * L
    # a disc that rides along the leg with the straight-line guess: every interior node starts at its centre (d = 0) and leaves along
    # the leg's left normal, to 1.01 R
    W = np.zeros((N, 5)); W[:, :2] = pb.p0[:2] + np.linspace(0, 1, N)[:, None] * leg; W[:, 4] = 12.0
    ride = KM.Track((0.0, T), (pb.p0[:2], pb.p1[:2]), R)
    ctr, Rr = KM.centres([ride], 0.0, N, K.H0)
    Ws = KM.start(pb, W, ctr, Rr)
    d = Ws[1:-1, :2] - ctr[0, 1:-1]
    assert np.allclose(np.hypot(*d.T), 1.01 * R, rtol=1e-12) and (d @ np.array([-ax[1], ax[0]]) > 0).all()
    assert KM.refused(pb, ctr, Rr, Ws)                                  # ... but the end poses lie at its centre: refused
    # an end pose inside the disc at node N - 1's time, although the disc's first knot is far away; and the reverse
    far = pb.p1[:2] + np.array([0.0, 10.0 * R])
    arrive = KM.Track((0.0, T), (far, pb.p1[:2] + 0.2 * R), R)
    leave = KM.Track((0.0, T), (pb.p1[:2] + 0.2 * R, far), R)
    assert KM.solve_moving(pb, W0, [arrive])[1]['status'] == KM.ST_NONFINITE
    assert K.solve(K.Plain(pb), W0, [(far[0], far[1], R)])[1]['status'] != KM.ST_NONFINITE
    assert KM.solve_moving(pb, W0, [leave])[1]['status'] != KM.ST_NONFINITE
    assert K.solve(K.Plain(pb), W0, [(pb.p1[0] + 0.2 * R, pb.p1[1] + 0.2 * R, R)])[1]['status'] == KM.ST_NONFINITE
    assert KM.solve_moving(pb, W0, [KM.Track((0.0, T), (far, far), np.nan)])[1]['status'] == KM.ST_NONFINITE
    Wn, info = KM.solve_moving(pb, W0, [arrive])
    assert np.array_equal(Wn, W0) and np.isnan(info['cost']) and info['inner'] == 0


def test_full_solves_hold_the_margin_continuously():
    import d2d.opty_utils as ou
    for N in KM.FULL_N:
        for prob, r, W0, trs, ko in KM.full_launch(N):
            W, info = KM.solve_moving(prob.pb, W0, trs, KM.FULL_T_START)
            t = KM.FULL_T_START + np.arange(N) * K.H0
            cl = ou.moving_keep_clearance([ko], t, W[:, 0], W[:, 1])[0]
            Wf, _ = nlp.solve(prob.pb, W0)
            clf = ou.moving_keep_clearance([ko], t, Wf[:, 0], Wf[:, 1])[0]
            print(f'{N}: status {info["status"]}, steps {info["inner"]}, cost {info["cost"]:.9f}, clearance {cl:.4f} (margin {ko.margin:.4f}); without the disc {clf:.4f}')
            assert info['status'] == 1 and cl >= ko.margin and clf < ko.margin
            assert info['zk'][0].max() > 0 and not info['zk'][0][[0, -1]].any()


def test_soft_ends_below_d_sep_and_hard_at_or_above_it():
    """Scenario 1 of tests/test_gpu_deconflict.py, margin 0: the sentence of the change."""
    import fleet_audit_ref as FL
    import fleet_tracks_ref as FT
    import nlp_moving_ref as M
    from test_gpu_deconflict import scenario, N, H, D_SEP, D_LOOK, STEP_MAX
    rows, n_ac = scenario(1)
    Wc = [nlp.solve(nlp.problem_from_row(r, N, H), M.straight_guess(r, N))[0] for r in rows]
    near = lambda Ws: FL.audit(np.stack(Ws, axis=2), n_ac, H, D_LOOK, STEP_MAX)['near_dist']        # noqa: E731
    Ws, _ = FT.deconflict(rows, Wc, n_ac, H, D_SEP, 0.0, D_LOOK, STEP_MAX)
    Wh, info = KM.deconflict_hard(rows, Wc, n_ac, H, D_SEP, 0.0, D_LOOK, STEP_MAX)
    print(f'independent {near(Wc).min():.4f} m, soft {near(Ws).min():.4f} m, hard {near(Wh).min():.4f} m (d_sep {D_SEP} m); hard: {info["replanned"]}, status {info["status"]}')
    assert near(Wc).min() < 1.0 and near(Ws).min() < D_SEP and abs(near(Ws).min() - 2.856) < 1e-3
    assert near(Wh).min() >= D_SEP and info['replanned'] == [[1]] and info['refused'] == [] and info['not_converged'] == []
    assert np.array_equal(Wh[0], Wc[0])                                  # the formation that outranks keeps its plan
    # the node distance sits on the constraint: R = sqrt(d_sep^2 + step_max^2) + chord_err
    R = KM.hard_radius(D_SEP, 0.0, STEP_MAX) + info['tracks'][0]['chord_err'][1, 0]
    dn = np.hypot(Wh[0][:, 0] - Wh[1][:, 0], Wh[0][:, 1] - Wh[1][:, 1]).min()
    assert abs(dn - R) <= 1e-6 * R


def moving_disc_across(e, v=(0.0, 1.5)):
    """tests/test_nlp_keepout_cpu.py's disc across exp_14's free plan (5 m, margin 1 m, centre (2.88, -4.54)), MOVING with velocity v and
    at that centre in the middle of the scenario's time span."""
    import d2d.opty_utils as ou
    tm = 0.5 * (e.t0 + e.t1)
    return ou.MovingKeepOut.linear(np.array((2.88, -4.54)) - np.array(v) * (tm - (e.t0 - 1.0)), v, 5.0, t0=e.t0 - 1.0, t1=e.t1 + 1.0, margin=1.0)


def test_planner_with_a_moving_keep_out_builds_its_tables_and_refuses_by_name():
    import d2d.optyplan_scenarios as sc
    import d2d.opty_utils as ou
    import single_opt_planner as sop
    from test_nlp_keepout_cpu import _exp14
    mk = moving_disc_across(sc.exp_14)
    st = ou.KeepOut((40.0, 40.0), 2.0)
    p = sop.Planner(_exp14(keep_out=[mk, st]), backend='auto')            # (no device is touched before run())
    assert p.prob.keep_moving and p.prob.keep_knots.shape == (2, 2, 3) and p.prob.keep_disc.shape == (2, 2)
    v_max = sc.exp_14.v_constraint[1]
    assert p.prob.keep_disc[0, 0] == mk.lowered(v_max, p.time_step) and p.prob.keep_disc[1, 0] == st.lowered(v_max, p.time_step)[2]
    assert (p.prob.keep_knots[1, :, 1:] == (40.0, 40.0)).all()
    assert not sop.Planner(_exp14(keep_out=[st]), backend='nlp').prob.keep_moving      # static lists keep their entry
    with pytest.raises(NotImplementedError, match="backend='fit'"):
        sop.Planner(_exp14(keep_out=[mk]), backend='fit')
    with pytest.raises(NotImplementedError, match='moving obstacles'):
        sop.Planner(_exp14(keep_out=[mk], moving_obstacles=[ou.MovingObstacle.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), backend='nlp')
    with pytest.raises(NotImplementedError, match='waypoints'):
        sop.Planner(_exp14(keep_out=[mk], waypoints=[ou.Waypoint(sc.exp_14.t0 + 1.0, x=1.0)]), backend='nlp')
    with pytest.raises(NotImplementedError, match='t1_free'):
        sop.Planner(_exp14(keep_out=[mk], t1_free=(sc.exp_14.t1 - 1.0, sc.exp_14.t1 + 1.0)), backend='nlp')

    class Odd:
        def cost(self, free, planner):
            return float(np.sum(free ** 2))

        def cost_grad(self, free, planner):
            return 2.0 * free
    with pytest.raises(NotImplementedError, match='keep_out together with a host objective'):
        sop.Planner(_exp14(keep_out=[mk], cost=Odd()), backend='nlp')


def test_header_version_and_binding():
    import d2dhip
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 126
    for name in ('d2d_nlp_solve_keepout_moving', 'd2d_nlp_solve_groups_keepout'):
        assert name in d2dhip.EXPORTS and re.search(rf'int {name}\(', hdr)
    assert int(re.search(r'#define D2D_MAX_MOV (\d+)', hdr).group(1)) == int(re.search(r'#define D2D_MAX_KEEP (\d+)', hdr).group(1)) == KM.MAX_MOV
