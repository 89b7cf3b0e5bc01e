"""GPU: how a fit ends badly, on every kernel of the trajectory-fit family (include/d2d.h, "Terminal states of a fit").

  a  a batch with four bad rows -- NaN end pose, inf start pose, NaN wind, a finite row whose cost overflows -- against the same batch
     with healthy rows in their places: the bad fits are refused (D2D_ST_NONFINITE, 0 trials, the non-finite cost of the first
     evaluation, q bit for bit the caller's), the healthy ones do not notice, the statistics leave the refusals out;
  b  the same through begin / iterate / finish: the loop on n_running ends, the exports are those of the one-call solve;
  c  refusals under the predicted hand-out (a batch past the resident wavefronts: the key of a NaN row);
  d  the trial cap, max_iter = 1, 2, 5: D2D_ST_MAXITER with iters == max_iter, the last accepted point, its cost -- by the oracle's cost
     function, by the evaluation kernel, and fit by fit by the oracle's solvers under the same cap;
  e  a coupled group with a NaN end pose: the group is refused whole, the others do not notice.

Inputs and the oracle's side: tests/fit_terminal_ref.py (tests/test_fit_terminal_cpu.py states the same contract without a GPU).
Every case asserts plan.kernel: no case can pass on another kernel than the one it names."""
import numpy as np
import pytest

import fit_terminal_ref as R
from oracle import fit as F, fit_knot as FK

pytestmark = pytest.mark.gpu
TOL = 1e-6                      # the suite's tolerance between a kernel and the oracle's fp32 split (tests/test_gpu_knot.py)
ST_CONVERGED, ST_MAXITER, ST_NONFINITE, ST_STALLED, ST_RUNNING = F.ST_CONVERGED, F.ST_MAXITER, F.ST_NONFINITE, F.ST_STALLED, F.ST_RUNNING
HEALTHY = [b for b in range(R.B_REFUSE) if b not in R.BAD_ROWS]
FIELDS = ('cost', 'q', 'iters', 'status')


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def plans(ctx):
    """name -> (plan, the oracle's basis from the plan's own arrays, its knot statement or None), built on first use"""
    import d2dhip
    made = {}

    def get(name):
        if name not in made:
            S, K, dur, wref = R.plan_consts(name)
            plan = d2dhip.FitPlan(ctx, S, K, dur, wref, kernel=R.PLANS[name][2])
            basis = F.FitBasis.from_arrays(S, K, dur, *plan.basis())
            made[name] = (plan, basis, FK.KnotBasis(basis) if R.PLANS[name][3] == 'knot' else None)
        assert made[name][0].kernel == R.PLANS[name][3], (name, made[name][0].kernel)
        return made[name]
    yield get
    for plan, _, _ in made.values():
        plan.close()


def _out(q, res):
    cost, iters, status, stats = res
    return {'cost': cost.cpu().numpy(), 'q': q.cpu().numpy(), 'iters': iters.cpu().numpy(), 'status': status.cpu().numpy(),
            'stats': np.array(stats, dtype=np.float64)}


def _solve(plan, dsc, q0, **kw):
    q = q0.clone()
    return _out(q, plan.solve(dsc, q, **kw))


def _solve_in_parts(plan, dsc, q0, per_call=7, max_calls=60, **kw):
    """begin / iterate (per_call trials a call, until nothing runs: a hard bound on the calls) / finish"""
    q = q0.clone()
    plan.begin(q0.shape[0])
    counts = []
    for _ in range(max_calls):
        counts.append(plan.iterate(dsc, q, per_call, **kw))
        if counts[-1] == 0:
            break
    assert counts[-1] == 0, 'the loop on n_running did not end: %s' % counts
    return _out(q, plan.finish(dsc, q)), counts


def _same(a, b, rows, what):
    for k in FIELDS:
        x, y = a[k][rows], b[k][rows]
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), '%s: %s differs in rows %s' % (
            what, k, np.nonzero((x != y).reshape(len(x), -1).any(1))[0][:8].tolist())


def _refusal_setup(ctx, plan, basis, name):
    """device rows of the healthy launch G and of the launch X with the four bad rows; the start points (plan.init of G) for both"""
    G0 = R.scenarios(name, R.B_REFUSE)
    for b in R.BAD_ROWS:
        G0[b] = G0[R.HEALTHY_SRC]
    q0 = plan.init(ctx.dev(G0))
    q0h = q0.cpu().numpy()
    assert np.isfinite(q0h).all()
    G, X = R.refusal_batches(name, basis, q0h)
    assert np.array_equal(G, G0)
    return G, X, q0, q0h


def _check_refused(out, q0h, X, basis, rows_kinds, what):
    for b, kind in rows_kinds:
        c = out['cost'][b]
        print('%s row %d (%s): status %d iters %d cost %r' % (what, b, kind, out['status'][b], out['iters'][b], c))
        assert out['status'][b] == ST_NONFINITE and out['iters'][b] == 0, (what, b, kind, out['status'][b], out['iters'][b])
        if kind == 'overflow':
            assert np.isposinf(R.start_cost(basis, X[b], q0h[b])) and np.isposinf(c), (what, kind, c)
        else:
            assert np.isnan(c), (what, kind, c)
        assert out['q'][b].tobytes() == q0h[b].tobytes(), (what, b, kind)      # (q0 is finite: no NaN-equals-NaN)


@pytest.mark.parametrize('name,mode', R.CASES)
def test_bad_rows_are_refused_and_their_neighbours_do_not_notice(ctx, plans, name, mode):
    plan, basis, _ = plans(name)
    kw = R.mode_kw(mode)
    G, X, q0, q0h = _refusal_setup(ctx, plan, basis, name)
    g = _solve(plan, ctx.dev(G), q0, **kw)
    x = _solve(plan, ctx.dev(X), q0, **kw)
    assert plan.kernel == R.PLANS[name][3]
    assert (g['status'] != ST_NONFINITE).all() and (g['status'] != ST_RUNNING).all() and np.isfinite(g['cost']).all()
    _same(x, g, HEALTHY, 'beside four refused fits')
    _check_refused(x, q0h, X, basis, list(zip(R.BAD_ROWS, R.KINDS)), '%s/%s' % (name, mode))
    # the statistics: refusals are counted among the unsettled fits and leave the sums alone
    n_unsettled = int(((g['status'] != ST_CONVERGED) & (g['status'] != ST_STALLED)).sum())
    n_bad_src = int(g['status'][R.HEALTHY_SRC] not in (ST_CONVERGED, ST_STALLED)) * len(R.BAD_ROWS)
    print('stats G', g['stats'], 'X', x['stats'])
    assert g['stats'][2] == n_unsettled and x['stats'][2] == len(R.BAD_ROWS) + n_unsettled - n_bad_src
    assert np.isfinite(x['stats'][0]) and 0.0 <= x['stats'][1] <= g['stats'][1]      # (the largest |J^T r| of the fits that were not refused)
    assert abs(x['stats'][0] - x['cost'][HEALTHY].sum()) <= 1e-12 * x['cost'][HEALTHY].sum()
    assert abs(g['stats'][0] - g['cost'].sum()) <= 1e-12 * g['cost'].sum()
    # ... and alone in the launch: B = 1, the one row bad
    for b, kind in zip(R.BAD_ROWS, R.KINDS):
        one = _solve(plan, ctx.dev(X[b:b + 1]), q0[b:b + 1], **kw)
        _check_refused(one, q0h[b:b + 1], X[b:b + 1], basis, [(0, kind)], '%s/%s B=1' % (name, mode))
        assert one['stats'][0] == 0.0 and np.isfinite(one['stats'][1]) and one['stats'][2] == 1.0


@pytest.mark.parametrize('name,mode', R.CASES)
def test_refusals_through_begin_iterate_finish(ctx, plans, name, mode):
    plan, basis, _ = plans(name)
    kw = R.mode_kw(mode)
    G, X, q0, q0h = _refusal_setup(ctx, plan, basis, name)
    dX = ctx.dev(X)
    slices = (0, 4) if R.PLANS[name][3] in ('knot', 'fused') and R.PLANS[name][1] == 50 else (0,)
    for sl in slices:
        kws = dict(kw, slice=sl) if sl else kw
        one = _solve(plan, dX, q0, **kws)
        parts, counts = _solve_in_parts(plan, dX, q0, **kws)
        assert plan.kernel == R.PLANS[name][3]
        print('%s/%s slice %d: running after each call %s' % (name, mode, sl, counts))
        assert counts[0] <= len(HEALTHY)                   # a refused fit is never RUNNING: not counted after its first evaluation
        _same(parts, one, HEALTHY, 'parts against one call (slice %d)' % sl)
        for k in ('iters', 'status'):
            assert np.array_equal(parts[k], one[k])
        assert parts['q'].tobytes() == one['q'].tobytes()
        assert np.array_equal(np.isnan(parts['cost']), np.isnan(one['cost'])) and np.array_equal(np.isposinf(parts['cost']), np.isposinf(one['cost']))
        _check_refused(parts, q0h, X, basis, list(zip(R.BAD_ROWS, R.KINDS)), '%s/%s parts slice %d' % (name, mode, sl))
        assert parts['stats'][2] == one['stats'][2] and np.isfinite(parts['stats'][:2]).all()


def test_refusals_under_the_predicted_handout(ctx, plans):
    """B = 8 n_cu + 1: the first batch the default solver orders by predicted trial counts (fit_handout_key_kernel: the key of a
    row with a NaN end pose is NaN and is replaced there)."""
    import torch
    plan, basis, _ = plans('knot50')
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 8 * n_cu + 1
    G = R.scenarios('knot50', 4096)
    G = np.concatenate([G] * (B // len(G) + 1))[:B].copy()
    bad = (0, B // 2, B - 1)
    for b in bad:
        G[b] = G[R.HEALTHY_SRC]
    X = G.copy()
    X[list(bad), F.SC_X1] = np.nan
    q0 = plan.init(ctx.dev(G))
    q0h = q0.cpu().numpy()
    g = _solve(plan, ctx.dev(G), q0)
    order_g = plan.last_order(B)
    x = _solve(plan, ctx.dev(X), q0)
    order_x = plan.last_order(B)
    assert plan.kernel == 'knot'
    for o in (order_g, order_x):
        assert np.array_equal(np.sort(o), np.arange(B))
    healthy = np.setdiff1d(np.arange(B), bad)
    _same(x, g, healthy, 'ordered hand-out beside three refused fits')
    _check_refused(x, q0h, X, basis, [(b, 'nan_x1') for b in bad], 'predicted hand-out')
    assert (g['status'] != ST_NONFINITE).all()
    assert x['stats'][2] == g['stats'][2] + 3 - 3 * int(g['status'][R.HEALTHY_SRC] not in (ST_CONVERGED, ST_STALLED)) and np.isfinite(x['stats'][:2]).all()


@pytest.mark.parametrize('name,mode', R.CASES)
def test_the_trial_cap(ctx, plans, name, mode):
    plan, basis, kb = plans(name)
    kw = R.mode_kw(mode)
    sc = R.cap_batch(name)
    dsc = ctx.dev(sc)
    q0 = plan.init(dsc)
    # The cost at plan.init, twice: by the evaluation kernel, and by the solver kernel under test itself -- a solve whose gradient
    # tests hold at once (gtol = 1e300) stops at its first evaluation and reports that cost.  Descent is a statement in the solver's
    # own arithmetic: the knot kernel evaluates in knot coordinates (u = u0 + Binv q), where the cost of the SAME point differs from
    # the q statement's by rounding -- measured 4.9e-12 relative at K = 50, inside the 1e-10 the suite asks of that identity
    # (tests/test_gpu_knot.py) and outside the 1e-12 of the descent test, which a fit whose first trial is rejected meets with equality.
    c_eval = plan.eval(dsc, q0, want_H=False)[0].cpu().numpy()
    own = _solve(plan, dsc, q0, max_iter=1, gtol=1e300, mp_tol=1e300, **kw)
    c_init = own['cost']
    print('%s/%s: the solver\'s cost at plan.init against the evaluation kernel\'s: largest relative difference %.3e' % (name, mode, np.abs(c_init / c_eval - 1.0).max()))
    assert (own['status'] == ST_CONVERGED).all() and (own['iters'] <= 1).all() and (np.abs(c_init - c_eval) <= 1e-10 * c_eval).all()
    rows, qs = R.sample_fits(name, mode)
    drows, dqs = ctx.dev(rows), ctx.dev(qs)
    for cap in R.CAPS:
        o = _solve(plan, dsc, q0, max_iter=cap, **kw)
        assert plan.kernel == R.PLANS[name][3]
        st, it = o['status'], o['iters']
        print('%s/%s cap %d: %d capped, %d converged, %d stalled' % (name, mode, cap, (st == ST_MAXITER).sum(), (st == ST_CONVERGED).sum(), (st == ST_STALLED).sum()))
        assert np.isin(st, (ST_CONVERGED, ST_STALLED, ST_MAXITER)).all()
        assert (it[st == ST_MAXITER] == cap).all() and (it <= cap).all()
        assert (st == ST_MAXITER).sum() * 3 >= len(st)
        c_or = np.array([F.cost(basis, sc[i], o['q'][i]) for i in range(len(sc))])
        assert np.abs(o['cost'] - c_or).max() <= 1e-10 * c_or.max() and (np.abs(o['cost'] - c_or) <= 1e-10 * c_or).all()
        ex = o['cost'] / c_init - 1.0
        print('%s/%s cap %d: largest cost / cost at plan.init - 1 = %.3e (fit %d, status %d, iters %d); %d fits above 0' % (
            name, mode, cap, ex.max(), ex.argmax(), st[ex.argmax()], it[ex.argmax()], (ex > 0).sum()))
        assert (o['cost'] <= c_init * (1 + 1e-12)).all()
        c_ev = plan.eval(dsc, ctx.dev(o['q']), want_H=False)[0].cpu().numpy()
        assert (np.abs(c_ev - o['cost']) <= 1e-10 * o['cost']).all()
        assert o['stats'][2] == (st == ST_MAXITER).sum()
        # fit by fit against the oracle under the same cap, in the kernel's precision split
        s = _solve(plan, drows, dqs, max_iter=cap, **kw)
        out = []
        for i in range(12):
            ref = R.oracle_solve(name, mode, basis, rows[i], qs[i], cap, True, kb)
            got = (s['q'][i], s['cost'][i], int(s['iters'][i]), int(s['status'][i]))
            if not (R.agree(got, ref, TOL) and (got[3] != ST_MAXITER or got[2] == ref[2] == cap)):
                out.append((i, got[3], ref[3], got[2], ref[2], abs(got[1] - ref[1]) / ref[1], np.abs(got[0] - ref[0]).max() / np.abs(ref[0]).max()))
        print('%s/%s cap %d: outside the oracle\'s %g: %s' % (name, mode, cap, TOL, out))
        assert len(out) <= 1, out
        assert (s['iters'][s['status'] == ST_MAXITER] == cap).all() and (s['status'] == ST_MAXITER).sum() >= 4
        if cap == 5:
            assert (s['status'] == ST_CONVERGED).sum() >= 1
    # a solve capped at 5 by max_iter == a solve given 5 trials by d2d_fit_iterate's budget and finished: q and cost bit for bit,
    # the fits the cap stopped exported as they stand (D2D_ST_RUNNING)
    capped = _solve(plan, dsc, q0, max_iter=5, **kw)
    q = q0.clone()
    plan.begin(len(sc))
    running = plan.iterate(dsc, q, 5, max_iter=200, **kw)
    fin = _out(q, plan.finish(dsc, q))
    assert fin['q'].tobytes() == capped['q'].tobytes() and fin['cost'].tobytes() == capped['cost'].tobytes()
    assert np.array_equal(fin['iters'], capped['iters'])
    was_capped = capped['status'] == ST_MAXITER
    assert running == was_capped.sum() and (fin['status'][was_capped] == ST_RUNNING).all()
    assert np.array_equal(fin['status'][~was_capped], capped['status'][~was_capped]) and fin['stats'][2] == was_capped.sum()
    # ... and d2d_fit_iterate at the cap says that nothing runs, however often it is asked
    q = q0.clone()
    plan.begin(len(sc))
    assert plan.iterate(dsc, q, 5, max_iter=5, **kw) == 0 and plan.iterate(dsc, q, 5, max_iter=5, **kw) == 0
    fin = _out(q, plan.finish(dsc, q))
    _same(fin, capped, list(range(len(sc))), 'iterate to the cap against the capped solve')


@pytest.mark.parametrize('bad_ac', [0, 1])
def test_a_coupled_group_with_a_nan_end_pose_is_refused_whole(ctx, bad_ac):
    import d2dhip
    from d2dhip import synth
    S, K, dur, wref = R.plan_consts('knot50')
    n_ac, n_grp, bad_grp, max_sweeps = 2, 6, 2, 60
    plan = d2dhip.FitPlan(ctx, S, K, dur, wref)
    try:
        assert plan.kernel == 'knot'
        plan.set_groups(n_ac)
        G = synth.circle_group_scenarios(n_ac, n_grp, dur, K, seed=1, obj_scale=1.0).reshape(n_grp * n_ac, -1)
        X = G.copy()
        X[bad_grp * n_ac + bad_ac, F.SC_X1] = np.nan
        q0 = plan.init(ctx.dev(G))
        q0h = q0.cpu().numpy()
        res = {}
        for key, rows in (('g', G), ('x', X)):
            q = q0.clone()
            cost, sweeps, stats = plan.solve_groups(ctx.dev(rows), q, n_ac, max_sweeps=max_sweeps, inner_iters=8, tol=1e-9)
            sw, mv = plan.group_report(n_grp)
            res[key] = (q.cpu().numpy(), cost.cpu().numpy(), sweeps, np.array(stats), sw, mv)
        (qg, cg, sg, stg, swg, mvg), (qx, cx, sx, stx, swx, mvx) = res['g'], res['x']
        print('sweeps G', swg, 'X', swx, 'moved X', mvx, 'costs of the refused group', cx[bad_grp * n_ac:(bad_grp + 1) * n_ac], 'stats', stx)
        mine = list(range(bad_grp * n_ac, (bad_grp + 1) * n_ac))
        others = [b for b in range(n_grp * n_ac) if b not in mine]
        og = [r for r in range(n_grp) if r != bad_grp]
        # the refused group: both aircraft untouched (the partner's collision rows read NaN positions), no sweep, a NaN move
        assert np.isfinite(q0h).all() and qx[mine].tobytes() == q0h[mine].tobytes()
        assert not np.isfinite(cx[mine]).any()
        assert swx[bad_grp] == 0 and np.isnan(mvx[bad_grp])
        # the five others: bit for bit the launch with a healthy row in that place; the sweep loop ends
        assert qx[others].tobytes() == qg[others].tobytes() and cx[others].tobytes() == cg[others].tobytes()
        assert np.array_equal(swx[og], swg[og]) and mvx[og].tobytes() == mvg[og].tobytes()
        assert (swg >= 1).all() and (swg <= max_sweeps).all() and sx == swx.max() <= max_sweeps
        assert np.isfinite(stx).all() and abs(stx[0] - cx[others].sum()) <= 1e-12 * cx[others].sum() and stx[2] == mvx[og].max()
    finally:
        plan.close()
