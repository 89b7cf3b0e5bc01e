"""GPU: full_sim.deconflict_plans and plan_batch(backend='nlp', deconflict=...) on two small shared worlds, against the loop's CPU
statement (fleet_tracks_ref.deconflict: the reference tracks plus the collocation statements of tests/nlp_moving_ref.py).

Scenario 1: two single aircraft (n_ac = 1), 41 nodes, h = 0.1 s, 48 m legs at 12 m/s that cross at the origin at node 20.
Scenario 2: three formations of three, aircraft 20 m apart.  Aircraft 0 of formation 0 (east along y = 0) and aircraft 0 of formation 1
(north along x = 0) meet at the origin at node 20; aircraft 2 of formation 1 (north along x = -40) and aircraft 0 of formation 2 (east
along y = 0 from x = -64) meet at (-40, 0) at node 20; no other pair comes within 14 m.  Two pairs of formations conflict, in a chain.

The moving discs are a soft cost.  With the rows' obstacle weight KOBS = 100 (kind 1), d_sep = 4 m and margin = 4 m the CPU statement,
run on its own, ends both scenarios at 4.237 m for every aircraft that was in conflict (margin 2 m: 3.79 m; KOBS = 10, margin 6 m:
3.10 m) in 1 and 2 rounds: that margin is used here and the bar near_dist >= d_sep is asserted for every aircraft.  Tolerances against
the CPU statement: those of tests/test_gpu_moving_obstacles.py -- status equal, cost within 1e-7 relative (of max(cost, 1e-3)), nodes
within 1e-4."""
import numpy as np
import pytest

import fleet_tracks_ref as FT
import nlp_moving_ref as M
from oracle import nlp

pytestmark = pytest.mark.gpu
N, H = 41, 0.1
D_SEP, MARGIN, D_LOOK, STEP_MAX, KOBS = 4.0, 4.0, 10.0, 2.0, 100.0
DEC = dict(d_sep=D_SEP, margin=MARGIN, d_look=D_LOOK, step_max=STEP_MAX)
UP = np.pi / 2


def scenario(k):
    """-> rows (R n_ac, SCEN_STRIDE), n_ac."""
    row = lambda p0, p1: M.row(1, p0=p0, p1=p1, N=N, kobs=KOBS)           # noqa: E731
    if k == 1:
        return np.stack([row((-24., 0., 0.), (24., 0., 0.)), row((0., -24., UP), (0., 24., UP))]), 1
    rows = [row((-24., 20. * a, 0.), (24., 20. * a, 0.)) for a in range(3)]
    rows += [row((-20. * b, -24., UP), (-20. * b, 24., UP)) for b in range(3)]
    rows += [row((-64., -20. * c, 0.), (-16., -20. * c, 0.)) for c in range(3)]
    return np.stack(rows), 3


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    return d2dhip.default_context()


@pytest.fixture(scope='module', params=[1, 2])
def case(request, ctx):
    """The scenario, its independent plans and its deconflicted plans through plan_batch, and the CPU statement -- each made once."""
    import full_sim
    rows, n_ac = scenario(request.param)
    W0 = np.stack([M.straight_guess(r, N).T for r in rows])
    plan = lambda **kw: full_sim.plan_batch(rows, N, (N - 1) * H, 1.0, backend='nlp', W0=W0, h=H, n_ac=n_ac, **kw)      # noqa: E731
    indep = plan()
    ctx.sync()
    Wi = indep['W'].cpu().numpy()
    out = plan(deconflict=DEC)
    ctx.sync()
    Wc = [nlp.solve(nlp.problem_from_row(r, N, H), M.straight_guess(r, N))[0] for r in rows]
    Wr, ref = FT.deconflict(rows, Wc, n_ac, H, D_SEP, MARGIN, D_LOOK, STEP_MAX)
    return dict(k=request.param, rows=rows, n_ac=n_ac, R=len(rows) // n_ac, W0=W0, indep=indep, Wi=Wi, out=out, W=out['W'].cpu().numpy(),
                info=out['deconflict'], Wr=Wr, ref=ref)


def _audit(ctx, W, n_ac, **kw):
    a = ctx.fleet_audit(W, n_ac, H, D_LOOK, STEP_MAX, d_safe=D_SEP, layout='plan', **kw)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in a.items()}


def test_the_independent_plans_conflict_and_none_changes_nothing(ctx, case):
    """Before: the audit finds the meeting; plan_batch(deconflict=None) is the direct solve, bit for bit."""
    before = _audit(ctx, case['indep']['W'], case['n_ac'])
    print('before', before['near_dist'])
    assert np.nanmin(before['near_dist']) < D_SEP and (before['near_dist'] < D_SEP).sum() == (2 if case['k'] == 1 else 4)
    W = ctx.dev(case['W0'].copy())
    direct = ctx.nlp_solve_groups(ctx.dev(case['rows']), W, H, n_ac=case['n_ac'])
    ctx.sync()
    assert W.cpu().numpy().tobytes() == case['Wi'].tobytes() and 'deconflict' not in case['indep']
    for k in ('cost', 'feas', 'iters', 'status'):
        assert direct[k].cpu().numpy().tobytes() == case['indep'][k].cpu().numpy().tobytes(), k


def test_priority_is_kept_and_the_bar_is_met(ctx, case):
    n_ac, R, W, Wi, info = case['n_ac'], case['R'], case['W'], case['Wi'], case['info']
    assert W[:n_ac].tobytes() == Wi[:n_ac].tobytes()                       # the top formation keeps its plan, byte for byte
    for f in range(1, R):                                                   # every lower formation had a partner: it changed
        assert np.abs(W[f * n_ac:(f + 1) * n_ac] - Wi[f * n_ac:(f + 1) * n_ac]).max() > 1.0, f
    assert info['rounds'] <= R - 1 and info['rounds'] == len(info['replanned']) and not info['truncated'] and info['not_converged'] == []
    mine = _audit(ctx, case['out']['W'], n_ac)
    for k in ('near_dist', 'near_partner', 'near_time', 'near_count', 'status'):
        assert mine[k].tobytes() == info['audit'][k].cpu().numpy().tobytes(), k
    print('after', mine['near_dist'])
    assert (mine['near_dist'] >= D_SEP).all() and info['unresolved'] == [] and (mine['near_count'] == 0).all()
    assert (info['tracks_status'].cpu().numpy() == 0).all()


def test_the_loop_is_the_cpu_statements(ctx, case):
    n_ac, info, ref = case['n_ac'], case['info'], case['ref']
    assert [s['forms'].cpu().numpy().tolist() for s in info['solves']] == ref['replanned'] == ([[1]] if case['k'] == 1 else [[1, 2], [2]])
    for s, costs, status in zip(info['solves'], ref['costs'], ref['status']):
        got, want = s['cost'].cpu().numpy(), np.concatenate(costs)
        rel = np.abs(got - want) / np.maximum(want, 1e-3)
        print('costs', got, want, 'rel', rel.max(), 'feas', s['feas'].cpu().numpy().max())
        assert (s['status'].cpu().numpy() == np.concatenate(status)).all() and (np.concatenate(status) == 1).all()
        assert rel.max() <= 1e-7 and s['feas'].cpu().numpy().max() <= 1e-8
    dn = max(np.abs(case['W'][b].T - case['Wr'][b]).max() for b in range(len(case['Wr'])))
    print('nodes', dn)
    assert dn <= 1e-4
    X = np.stack(case['Wr'], axis=2)
    import fleet_audit_ref as FL
    assert (FL.audit(X, n_ac, H, D_LOOK, STEP_MAX)['near_dist'] >= D_SEP).all()           # the statement alone reaches the bar


def test_a_second_world_on_top_changes_nothing(ctx, case):
    """The same formations twice, the copies in another world: both worlds end as the single world did, byte for byte."""
    import full_sim
    rows, n_ac, R = case['rows'], case['n_ac'], case['R']
    W = ctx.dev(np.concatenate([case['Wi'], case['Wi']]))
    _, info = full_sim.deconflict_plans(ctx, ctx.dev(np.concatenate([rows, rows])), W, H, n_ac, world=[0] * R + [7] * R, **DEC)
    ctx.sync()
    W = W.cpu().numpy()
    assert W[:R * n_ac].tobytes() == case['W'].tobytes() and W[R * n_ac:].tobytes() == case['W'].tobytes()
    assert info['replanned'] == [2 * n for n in case['info']['replanned']] and info['unresolved'] == []
    # ... and in ONE world the copies lie on top of each other: everybody but the first formation has partners at distance 0
    both = _audit(ctx, ctx.dev(np.concatenate([case['Wi'], case['Wi']])), n_ac)
    assert (both['near_dist'] == 0.0).all()
