"""GPU parity: collocation plans through timed waypoints (d2d_nlp_solve_via, d2d_nlp_solve_groups_via; csrc/nlp_kernels.hip, the VIA
instantiations) against
  * the CPU statement tests/nlp_via_ref.py (oracle.nlp.solve / nlp_wind_ref.solve / nlp_groups_pairs_ref.solve_groups on Problems
    with lo == hi on the pinned components), end of solve and Newton step by Newton step,
  * the entries without pins, bit for bit when no row pins anything,
and the refusals and the host routing on top.  Tolerances: those of tests/test_gpu_moving_obstacles.py -- status equal,
feas <= 1e-8, cost within 1e-7 relative, nodes within 1e-4 -- and the pinned components of the returned W equal their values exactly."""
import functools

import numpy as np
import pytest

import nlp_groups_pairs_ref as P
import nlp_moving_ref as M
import nlp_steps_ref as S
import nlp_via_ref as V
import nlp_wind_ref as R
from d2d.opty_utils import MovingObstacle, Waypoint, waypoint_error
from oracle import nlp

pytestmark = pytest.mark.gpu
N, H = V.N_NODES, V.H


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return R.fields()


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if k in ('cost', 'feas', 'iters', 'status', 'sweeps', 'moved', 'mult', 'via_work')
            and v is not None}


def _solve(ctx, rows, W0, tabs, field=None, t_start=None, moving=None, h=H, **kw):
    """rows (B, SCEN_STRIDE), W0 (B, 5, N), tabs: one table per problem (or None: no via argument) -> W (B, 5, N), outputs as numpy."""
    W = ctx.dev(np.ascontiguousarray(W0)); dsc = ctx.dev(np.ascontiguousarray(rows))
    kn, dc = M.tables(moving) if moving is not None else (None, None)
    t = None if t_start is None else ctx.dev(np.ascontiguousarray(np.asarray(t_start, dtype=np.float64)))
    via = None if tabs is None else ctx.dev(np.ascontiguousarray(V.tables(tabs)))
    out = ctx.nlp_solve_via(dsc, W, h, via, None if kn is None else ctx.dev(kn), None if dc is None else ctx.dev(dc), field, t, **kw)
    ctx.sync()
    return W.cpu().numpy(), _np(out)


def _groups(ctx, rows, W0, tabs, field=None, t_start=None, n_ac=P.N_AC, **kw):
    W = ctx.dev(np.ascontiguousarray(W0)); dsc = ctx.dev(np.ascontiguousarray(rows))
    t = None if t_start is None else ctx.dev(np.ascontiguousarray(np.asarray(t_start, dtype=np.float64)))
    via = None if tabs is None else ctx.dev(np.ascontiguousarray(V.tables(tabs)))
    out = ctx.nlp_solve_groups_via(dsc, W, H, n_ac, via, None, None, field, t, **kw)
    ctx.sync()
    return W.cpu().numpy(), _np(out)


def _check(tag, W, out, b, Wo, info, tab):
    rel = abs(out['cost'][b] - info['cost']) / max(info['cost'], 1e-3)
    dn = np.abs(W[b].T - Wo).max()
    print(f'{tag}: status {out["status"][b]} / {info["status"]}, cost rel {rel:.2e}, nodes {dn:.2e}, feas {out["feas"][b]:.2e}, '
          f'steps {out["iters"][b]} / {info["inner"]}')
    assert out['status'][b] == info['status'] == 1
    assert out['feas'][b] <= 1e-8
    assert rel <= 1e-7
    assert dn <= 1e-4
    assert waypoint_error(tab, W[b]) == 0.0              # exactly


@pytest.mark.parametrize('wind', ['const', 'gust'])
@pytest.mark.parametrize('serial', [0, 1])
def test_catalogue_against_the_cpu_statement(ctx, fields, wind, serial):
    """1. The catalogue of one wind in one launch (every mask: x, y, psi, xy, xy psi; the first and the last interior node; a box),
    cyclic reduction and the twisted serial recursion."""
    cat = V.catalogue(wind)
    F, t0 = (None, None) if wind == 'const' else (fields['gust'], V.GUST_T_START)
    rows = np.stack([r for r, _ in cat.values()]); tabs = [t for _, t in cat.values()]
    assert {int(m) for t in tabs for m in t[:, 1]} >= {1, 2, 3, 4, 7}
    W0 = np.stack([V.guess(r, t).T for r, t in cat.values()])
    W, out = _solve(ctx, rows, W0, tabs, F, None if t0 is None else [t0] * len(rows), serial=serial)
    for b, (name, (r, tab)) in enumerate(cat.items()):
        Wo, info = V.solve(V.problem(r, tab), W0[b].T, F, t0 or 0.0)
        _check(f'{name} serial={serial}', W, out, b, Wo, info, tab)
        fixed = out['via_work'][b]
        assert fixed[0] == fixed[-1] == 7 and sorted(np.nonzero(fixed[1:-1])[0] + 1) == sorted({int(k) for k in tab[:, 0]})


@pytest.mark.parametrize('serial', [0, 1])
@pytest.mark.parametrize('name', list(V.shapes()))
def test_shapes_against_the_cpu_statement(ctx, name, serial):
    """2. N = 3 (no free position), 4 (two neighbouring fixed nodes), 7, 66 (three fixed nodes across the 64-lane chunk boundary), 121,
    130 (records in global memory), and the middle nodes of N = 61 where the serial recursion meets."""
    n, r, tab = V.shapes()[name]
    W0 = V.guess(r, tab, n)
    W, out = _solve(ctx, r[None], W0.T[None], [tab], serial=serial)
    Wo, info = V.solve(V.problem(r, tab, n), W0)
    _check(f'{name} serial={serial}', W, out, 0, Wo, info, tab)


def _step_case(cid, r, tab, n=N, field=None, t0=0.0, seed=1):
    pb = V.problem(r, tab, n)
    import d2dhip as D
    W0 = S._start(r[D.SC_X0:D.SC_X0 + 3], r[D.SC_X1:D.SC_X1 + 3], n, seed)
    if field is None:
        return S._single(cid, W0, functools.partial(nlp.solve, pb), lambda W: (nlp.cost(pb, W), float(np.abs(nlp.constraints(pb, W)).max())))
    fp = R.FieldProblem(pb, field, t0)
    return S._single(cid, W0, functools.partial(R.solve, fp), lambda W: (nlp.cost(pb, W), float(np.abs(R.constraints(fp, W)).max())))


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_single_solves_follow_the_statement_step_by_step(ctx, fields, wind):
    """3. nlp_steps_ref's comparison for a pinned problem: after every budget the step count is the statement's, and W and the
    multipliers (times 2 rho) agree to the tolerance measure() finds on the statement alone.  cost and feas are no comparison of two
    solves: they are the statement's own functions evaluated at the KERNEL's W, a self-consistency check of the kernel's report, held to
    1e-11 relative and 1e-12 absolute as tests/test_gpu_nlp_steps.py holds them (a sum of N terms of order one in fp64)."""
    F, t0 = (None, 0.0) if wind == 'const' else (fields['gust'], V.GUST_T_START)
    r, tab = V.catalogue(wind)['heading' if wind == 'const' else 'gust-heading']
    case = _step_case(f'via-{wind}-heading', r, tab, field=F, t0=t0)
    bad, worst = [], 0.0
    for budget in S.BUDGETS:
        m = S.measure(case, budget)
        info, tol = m['info']['raw'], m['tol']
        W, out = _solve(ctx, r[None], case.W0[0].T[None], [tab], F, None if F is None else [t0], want_mult=True,
                        inner_max=budget[0], outer_max=budget[1])
        Wk = W[0].T
        head = f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        err = float(np.abs(Wk - m['W'][0]).max()); worst = max(worst, err / tol)
        print(f'{head}: |W - statement| {err:.2e}, iters {out["iters"][0]} / {info["inner"]}')
        if int(out['iters'][0]) != info['inner']:
            bad.append(f'{head}: iters {out["iters"][0]}, the statement took {info["inner"]}')
        if not err <= tol:
            bad.append(f'{head}: W off by {err:.2e}')
        em = float(np.abs(2 * info['rho'] * out['mult'][0].T[1:] - info['mult']).max())
        if not em <= tol * 2 * info['rho']:
            bad.append(f'{head}: multipliers off by {em:.2e}')
        cost, feas = case.fn(Wk)
        if not (abs(out['cost'][0] - cost) <= 1e-11 * max(1.0, abs(cost)) and abs(out['feas'][0] - feas) <= 1e-12):
            bad.append(f'{head}: cost / feas {out["cost"][0]!r} {out["feas"][0]!r}, the statement at the same W {cost!r} {feas!r}')
        if waypoint_error(tab, W[0]) != 0.0:
            bad.append(f'{head}: a pin moved')
    print(f'{case.cid}: largest error / tol {worst:.2e}')
    assert not bad, '\n'.join(bad)


def test_group_solves_follow_the_statement_step_by_step(ctx):
    """3b. One four-aircraft scenario (all pairs coupled, two sweeps) with a pin on aircraft 0 and on aircraft 2: step counts, sweeps,
    W, the last move and the multipliers of every aircraft's last solve, to the tolerance of measure()."""
    sc = P.pair_scenarios()[0]
    pins = V.group_pins(sc)
    W0s = P.guesses(sc)

    def run(W0, inner_max, outer_max):          # nlp_steps_ref._scenario's, which also keeps rho and the multipliers of the last solves
        path = []

        def inner(a, pb, W):
            Wn, info = nlp.solve(pb, W, inner_max=inner_max, outer_max=outer_max)
            path.extend(info['path'])
            return Wn, info
        pbs = [V.pin(pb, tb) for pb, tb in zip(P.problems_of(sc), pins)]
        Ws, infos, sweeps, moved = P.solve_groups(pbs, [w for w in W0], inner, P.masks_of(sc), max_sweeps=2)
        return np.stack(Ws), dict(inner=tuple(i['inner'] for i in infos), status=tuple(i['status'] for i in infos), path=tuple(path),
                                  sweeps=sweeps, moved=moved, rho=tuple(i['rho'] for i in infos), mult=tuple(i['mult'] for i in infos))
    case = S.Case('via-groups-4-sweeps2-all', np.stack(W0s), run)
    bad = []
    for budget in S.BUDGETS:
        m = S.measure(case, budget)
        info, tol = m['info'], m['tol']
        W, out = _groups(ctx, sc, np.stack([w.T for w in W0s]), pins, max_sweeps=2, inner_max=budget[0], outer_max=budget[1], want_mult=True)
        head = f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        err = max(float(np.abs(W[a].T - m['W'][a]).max()) for a in range(P.N_AC))
        print(f'{head}: |W - statement| {err:.2e}, iters {tuple(out["iters"])} / {info["inner"]}')
        if tuple(int(i) for i in out['iters']) != info['inner'] or int(out['sweeps'][0]) != info['sweeps']:
            bad.append(f'{head}: iters {tuple(out["iters"])} sweeps {out["sweeps"][0]}, the statement {info["inner"]} {info["sweeps"]}')
        if not err <= tol:
            bad.append(f'{head}: W off by {err:.2e}')
        if not abs(out['moved'][0] - info['moved']) <= 2 * tol:
            bad.append(f'{head}: moved {out["moved"][0]!r}, the statement {info["moved"]!r}')
        for a in range(P.N_AC):
            em = float(np.abs(2 * info['rho'][a] * out['mult'][a].T[1:] - info['mult'][a]).max())
            if not em <= tol * 2 * info['rho'][a]:
                bad.append(f'{head}: aircraft {a}: multipliers off by {em:.2e} > {tol * 2 * info["rho"][a]:.2e}')
    assert not bad, '\n'.join(bad)


def _bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ('cost', 'feas', 'iters', 'status'))


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_no_pins_is_the_moving_entry_bit_for_bit(ctx, fields, wind):
    """4. n_via = 0 and tables whose masks are all 0 against nlp_solve_moving (and nlp_solve / nlp_solve_wind), with a moving disc."""
    F, t0, leg = (None, 0.0, M.LEG) if wind == 'const' else (fields['gust'], V.GUST_T_START, M.LEG_GUST)
    names = ('crossing', 'headon')
    rows = np.stack([M.row(1, p1=(leg, 0.0, 0.0))] * 2)
    mv = [M.catalogue(1, t0, leg)[n] for n in names]
    W0 = np.stack([M.straight_guess(r).T for r in rows])
    ts = [t0, t0]
    Wd = ctx.dev(W0.copy()); kn, dc = M.tables(mv)
    od = ctx.nlp_solve_moving(ctx.dev(rows), Wd, H, ctx.dev(kn), ctx.dev(dc), F, ctx.dev(np.array(ts)))
    ctx.sync()
    Wm, om = Wd.cpu().numpy(), _np(od)
    absent = [np.array([[30.0, 0.0, 1.0, 2.0, 3.0], [np.nan, 0.0, np.nan, np.nan, np.nan]])] * 2      # mask 0: nothing of the row is used
    for tag, tabs in (('n_via = 0', None), ('all masks 0', absent)):
        W, out = _solve(ctx, rows, W0, tabs, F, ts, mv)
        assert np.array_equal(W, Wm) and _bits(out, om), tag
    # nothing moves either: d2d_nlp_solve / d2d_nlp_solve_wind
    Wd = ctx.dev(W0.copy())
    od = ctx.nlp_solve(ctx.dev(rows), Wd, H) if F is None else ctx.nlp_solve_wind(ctx.dev(rows), Wd, H, F, t_start=t0)
    ctx.sync()
    W, out = _solve(ctx, rows, W0, absent, F, None if F is None else ts)
    assert np.array_equal(W, Wd.cpu().numpy()) and _bits(out, _np(od))


def test_groups_without_pins_is_the_groups_moving_entry_bit_for_bit(ctx):
    sc = P.pair_scenarios()[0]
    W0 = np.stack([w.T for w in P.guesses(sc)])
    Wd = ctx.dev(W0.copy())
    od = ctx.nlp_solve_groups_moving(ctx.dev(sc), Wd, H, P.N_AC, max_sweeps=3)
    ctx.sync()
    for tabs in (None, [np.zeros((2, 5))] * P.N_AC):
        W, out = _groups(ctx, sc, W0, tabs, max_sweeps=3)
        assert np.array_equal(W, Wd.cpu().numpy()) and _bits(out, _np(od)) and np.array_equal(out['sweeps'], od['sweeps'].cpu().numpy())


def test_batch_equals_each_problem_alone_and_repeats(ctx):
    """5. Eight pinned problems in one launch, each alone, and the launch again: bit for bit."""
    cat = list(V.catalogue('const').values())[:8]
    rows = np.stack([r for r, _ in cat]); tabs = [t for _, t in cat]
    W0 = np.stack([V.guess(r, t).T for r, t in cat])
    W, out = _solve(ctx, rows, W0, tabs)
    W2, out2 = _solve(ctx, rows, W0, tabs)
    assert np.array_equal(W, W2) and _bits(out, out2)
    n_via = V.tables(tabs).shape[1]
    for b in range(8):
        W1, o1 = _solve(ctx, rows[b:b + 1], W0[b:b + 1], [V.table(tabs[b], n_via)])
        assert np.array_equal(W1[0], W[b]) and all(o1[k][0] == out[k][b] for k in ('cost', 'feas', 'iters', 'status')), b


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_fewer_slots_than_problems_and_the_order_only_schedule(ctx, fields, wind):
    """6b. The hand-out loop of the via kernels: six problems of 41 nodes, the catalogue's pins moved to a 4 s leg (48 m in still air,
    32 m in the gust: point, heading, yonly, a pin on node 0, psionly, last), so problem 3 is unusable.  (a) index order, default
    slots; (b) two slots and the reversed order: a slot takes a third ticket, the refused problem lies between two solved ones -- W,
    cost, feas, iters, status equal (a) bitwise; (c) two slots and the order with problem 1's entry replaced by an index outside
    [0, B): the others equal (a) bitwise, problem 1 keeps its guess (its outputs are not written: compared only where defined).  The
    refused problem: ST_NONFINITE, NaN cost, W bitwise its guess, in every run."""
    import torch
    import d2dhip as D
    n, B, BAD, DROP = 41, 6, 3, 1
    OUT = ('cost', 'feas', 'iters', 'status')
    leg, t0, F, dy = (48.0, 0.0, None, 5.0) if wind == 'const' else (32.0, V.GUST_T_START, fields['gust'], 3.0)
    r = M.row(1, p1=(leg, 0.0, 0.0), N=n, kobs=0.0)
    mid, step = (n - 1) // 2, leg / (n - 1)
    tabs = [V.rows_of((mid, {0: leg / 2, 1: dy})), V.rows_of((mid, {0: leg / 2, 1: dy, 2: 0.0})), V.rows_of((mid, {1: 0.6 * dy})),
            V.rows_of((0, {0: 0.0, 1: 0.0})), V.rows_of((mid, {2: 0.2})), V.rows_of((n - 2, {0: leg - step, 1: 0.0}))]
    rows = np.stack([r] * B)
    W0 = np.stack([(V.guess(r, tab, n) if b != BAD else M.straight_guess(r, n)).T for b, tab in enumerate(tabs)])
    dsc, dvia = ctx.dev(rows), ctx.dev(np.ascontiguousarray(V.tables(tabs)))
    dts = None if F is None else ctx.dev(t0 + 0.25 * np.arange(B))

    def run(**kw):
        W = ctx.dev(W0.copy())
        out = ctx.nlp_solve_via(dsc, W, H, dvia, None, None, F, dts, **kw)
        ctx.sync()
        return W.cpu().numpy(), _np(out)

    def order(perm):
        return torch.from_numpy(np.asarray(perm, dtype=np.int32)).to(ctx.device)

    rev = np.arange(B)[::-1].copy()
    dropped = rev.copy(); dropped[rev == DROP] = -1
    Wa, oa = run()
    Wb, ob = run(slots=2, order=order(rev))
    Wc, oc = run(slots=2, order=order(dropped))
    print(f'{wind}: status {oa["status"]}, steps {oa["iters"]}')
    assert (np.delete(oa['status'], BAD) != D.ST_NONFINITE).all()
    assert Wb.tobytes() == Wa.tobytes() and all(ob[k].tobytes() == oa[k].tobytes() for k in OUT)
    keep = np.arange(B) != DROP
    assert Wc[keep].tobytes() == Wa[keep].tobytes() and all(oc[k][keep].tobytes() == oa[k][keep].tobytes() for k in OUT)
    assert np.array_equal(Wc[DROP], W0[DROP])
    for W, out in ((Wa, oa), (Wb, ob), (Wc, oc)):
        assert out['status'][BAD] == D.ST_NONFINITE and np.isnan(out['cost'][BAD]) and np.array_equal(W[BAD], W0[BAD])


def test_a_pin_on_the_unpinned_plan_changes_nothing(ctx):
    """6. Pinning node 30 where the unpinned solve passes gives that plan again, to the statement's tolerances."""
    r = M.row(1, p1=(M.LEG, 0.0, 0.0))
    mv = [M.catalogue(1, 0.0)['crossing']]
    W0 = M.straight_guess(r).T[None]
    Wu, ou = _solve(ctx, r[None], W0, None, None, [0.0], mv)
    tab = V.rows_of((30, {0: Wu[0, 0, 30], 1: Wu[0, 1, 30], 2: Wu[0, 2, 30]}))
    Wp, op = _solve(ctx, r[None], W0, [tab], None, [0.0], mv)
    print(f'pinned on the plan: nodes {np.abs(Wp - Wu).max():.2e}, cost {op["cost"][0]:.9f} / {ou["cost"][0]:.9f}')
    assert ou['status'][0] == op['status'][0] == 1 and np.abs(Wp - Wu).max() <= 1e-4
    assert abs(op['cost'][0] - ou['cost'][0]) <= 1e-7 * ou['cost'][0] and waypoint_error(tab, Wp[0]) == 0.0


def test_a_pin_with_a_static_disc_a_moving_disc_and_a_box(ctx):
    """7. The objective's terms still count at and around a pinned node; the pin lies inside an x / y box that is set."""
    import d2dhip as D
    r = V.boxed_row(M.row(1, p1=(M.LEG, 0.0, 0.0)), (-5.0, 80.0), (-12.0, 9.0))
    r[D.SC_O0X:D.SC_O0X + 3] = (54.0, 2.0, 4.0)
    mv = [MovingObstacle.linear((20.0, -20.0), (0.0, 10.0), 5.0, t0=0.0, t1=20.0)]
    tab = V.rows_of((30, {0: 36.0, 1: 8.0}))
    W0 = V.guess(r, tab)
    W, out = _solve(ctx, r[None], W0.T[None], [tab], None, [0.0], [mv])
    Wo, info = V.solve(V.problem(r, tab, moving=mv), W0)
    _check('pin + disc + moving disc + box', W, out, 0, Wo, info, tab)
    assert info['cost'] > V.COSTS['point'] + 1e-3        # the discs are felt


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_groups_against_the_cpu_statement(ctx, fields, wind):
    """8. nlp_groups_pairs_ref.pair_scenarios()[0], all six pairs coupled, with a pin on aircraft 0 and on aircraft 2."""
    sc = P.pair_scenarios()[0]
    pins = V.group_pins(sc)
    F, ts = (None, None) if wind == 'const' else (fields['gust'], [V.GUST_T_START])
    W0s = P.guesses(sc)
    W, out = _groups(ctx, sc, np.stack([w.T for w in W0s]), pins, F, ts, max_sweeps=P.MAX_SWEEPS)
    pbs = [V.pin(pb, tb) for pb, tb in zip(P.problems_of(sc), pins)]
    inner = P.in_constant_wind() if F is None else P.in_field(F, V.GUST_T_START)
    Ws, infos, sweeps, moved = P.solve_groups(pbs, W0s, inner, P.masks_of(sc), max_sweeps=P.MAX_SWEEPS)
    print(f'{wind}: sweeps {out["sweeps"][0]} / {sweeps}, moved {out["moved"][0]:.2e} / {moved:.2e}')
    assert out['sweeps'][0] == sweeps
    for a in range(P.N_AC):
        _check(f'{wind} aircraft {a}', W, out, a, Ws[a], infos[a], pins[a])


def test_malformed_tables_refuse_their_problem_alone(ctx):
    """9. Every refusal of the validation, one problem each, between two good neighbours that solve to the statement."""
    r, good = V.catalogue()['point']
    rb = V.boxed_row(r, (-5.0, 80.0), (-2.0, 9.0))
    bad = {'node 0': [[0, 3, 0, 0, 0]], 'node N-1': [[N - 1, 3, 72, 0, 0]], 'node 30.5': [[30.5, 3, 36, 8, 0]], 'node nan': [[np.nan, 1, 36, 8, 0]],
           'mask 8': [[30, 8, 36, 8, 0]], 'mask -1': [[30, -1, 36, 8, 0]], 'mask 1.5': [[30, 1.5, 36, 8, 0]], 'mask nan': [[30, np.nan, 36, 8, 0]],
           'value nan': [[30, 3, 36, np.nan, 0]], 'value inf': [[30, 4, 0, 0, np.inf]],
           'twice': [[30, 3, 36, 8, 0], [30, 6, 0, 8, 0.1]], 'outside the box': [[30, 3, 36, 9.5, 0]]}
    names = list(bad)
    rows = np.stack([r] + [rb if n == 'outside the box' else r for n in names] + [r])
    tabs = [good] + [np.array(bad[n], dtype=np.float64) for n in names] + [good]
    W0 = np.stack([V.guess(r, good).T] * len(rows))
    W, out = _solve(ctx, rows, W0, tabs)
    Wo, info = V.solve(V.problem(r, good), W0[0].T)
    for b in (0, len(rows) - 1):
        _check(f'good neighbour {b}', W, out, b, Wo, info, good)
    for b, n in enumerate(names, 1):
        assert out['status'][b] == 3 and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and out['iters'][b] == 0, n
        assert np.array_equal(W[b], W0[b]), n
    # a value whose component the mask leaves out is not read; the same node pinned by two rows in different components is fine
    ok = [np.array([[30, 1, 36, np.nan, np.nan], [30, 2, np.nan, 8, np.nan]])]
    W1, o1 = _solve(ctx, r[None], W0[:1], ok)
    assert o1['status'][0] == 1 and np.abs(W1[0] - W[0]).max() <= 1e-9


def test_a_bad_table_refuses_its_scenario(ctx):
    sc = P.pair_scenarios()[0]
    W0 = np.stack([w.T for w in P.guesses(sc)] * 2)
    pins = V.group_pins(sc)
    badp = [p.copy() for p in pins]; badp[2][0, 0] = 0.0
    W, out = _groups(ctx, np.concatenate([sc, sc]), W0, badp + pins, max_sweeps=2)
    Wg, og = _groups(ctx, sc, W0[:P.N_AC], pins, max_sweeps=2)
    assert (out['status'][:4] == 3).all() and np.isnan(out['cost'][:4]).all() and out['sweeps'][0] == 0 and np.array_equal(W[:4], W0[:4])
    assert np.array_equal(W[4:], Wg) and np.array_equal(out['cost'][4:], og['cost']) and out['sweeps'][1] == og['sweeps'][0]


def test_einval(ctx):
    import ctypes as C
    import d2dhip
    r, tab = V.catalogue()['point']
    dsc, W = ctx.dev(r[None]), ctx.dev(V.guess(r, tab).T[None].copy())
    with pytest.raises(d2dhip.D2DError, match='n_via'):
        ctx.nlp_solve_via(dsc, W, H, ctx.dev(np.zeros((1, d2dhip.MAX_VIA + 1, 5))))
    work = ctx.empty(ctx.lib.d2d_nlp_workspace_doubles(N)); cost, feas = ctx.empty(1), ctx.empty(1)
    vw = d2dhip._torch().zeros(N, dtype=d2dhip._torch().int32, device=W.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = (ctx.h, 1, N, H, p(dsc), None, p(W), p(work), None, p(cost), p(feas), None, None, None, None, None, None)
    v = d2dhip.ViaPointsC(1, ctx.dev(tab[None]).data_ptr())
    for via, vwork in ((None, p(vw)), (C.byref(d2dhip.ViaPointsC(-1, v.pts)), p(vw)), (C.byref(d2dhip.ViaPointsC(1, None)), p(vw)), (C.byref(v), None)):
        assert ctx.lib.d2d_nlp_solve_via(*args, via, vwork) != 0
        assert ctx.lib.d2d_nlp_solve_groups_via(ctx.h, 1, 1, N, H, p(dsc), None, 2, 1e-7, p(W), p(work), None, p(cost), p(feas), None, None, None, None,
                                                None, None, None, None, via, vwork) != 0
    ctx.sync()
    assert np.array_equal(W.cpu().numpy()[0], V.guess(r, tab).T)           # nothing was launched


def test_the_unreachable_point_stalls_like_the_statement(ctx):
    r, _ = V.catalogue()['point']
    W0 = V.guess(r, V.UNREACHABLE)
    W, out = _solve(ctx, r[None], W0.T[None], [V.UNREACHABLE])
    Wo, info = V.solve(V.problem(r, V.UNREACHABLE), W0)
    print(f'unreachable: status {out["status"][0]} / {info["status"]}, feas {out["feas"][0]!r} / {info["feas"]!r}')
    assert out['status'][0] == info['status'] == 4
    assert abs(out['feas'][0] - info['feas']) <= 1e-6 * info['feas'] and waypoint_error(V.UNREACHABLE, W[0]) == 0.0


def test_planner_problem_and_plan_batch_route_through_the_pins(ctx):
    """10. Planner(exp with waypoints), Problem.solve with a third instance time and plan_batch(via=): info['waypoint_error'] == 0.0."""
    import d2dhip
    import single_opt_planner as sop
    import multi_opt_planner as mop
    import full_sim as fs
    import d2d.multiopty_utils as d2mou

    class exp(sop.exp_1):
        p0 = (0., 0., 0., 0., 12.)
        t1, p1 = 6., (72., 0., 0., 0., 12.)
        waypoints = [Waypoint(3.0, 36.0, 8.0), Waypoint(4.5, psi=0.0)]
    p = sop.Planner(exp)
    p.run()
    assert p.info['backend_used'] == 'nlp' and p.info['status'] == 1 and p.info['waypoint_error'] == 0.0
    assert (p.sol_x[30], p.sol_y[30], p.sol_psi[45]) == (36.0, 8.0, 0.0)
    sol, info = p.prob.solve(p.get_initial_guess('via'))                   # the Problem itself, as the reference calls it
    assert info['status'] == 1 and info['waypoint_error'] == 0.0 and np.array_equal(sol, p.solution)

    class multi(mop.trap_4):
        p0s = ((0., 0., 0., 0., 12.), (0., 100., 0., 0., 12.)); p1s = ((60., 0., 0., 0., 12.), (60., 100., 0., 0., 12.)); t1 = 5.
        waypoints = [[Waypoint(2.5, 30.0, 3.0)], []]
        # (no collision term: what is looked at here is the routing, and the alternation of a pair re-solves each aircraft to 1e-6 only)
        cost = d2mou.CostComposit(kvel=70., kbank=1., kobs=float('nan'), kcol=float('nan'), vsp=12, obss=[], obs_kind=0, rcol=10)
    m = mop.Planner(multi)
    m.run()
    m.interpret_solution()
    assert m.info['backend_used'] == 'nlp' and m.info['waypoint_error'] == 0.0 and (m.sol_x[0][25], m.sol_y[0][25]) == (30.0, 3.0)
    assert list(m.info['status']) == [1, 1]
    r, tab = V.catalogue()['point']
    out = fs.plan_batch(np.stack([r, r]), N, 6.0, 1.0 / N, backend='nlp', W0=np.stack([V.guess(r, tab).T] * 2), h=H,
                        via=[[Waypoint(3.0, 36.0, 8.0)], []])
    st = out['status'].cpu().numpy()
    assert (st == 1).all() and out['waypoint_error'] == 0.0 and abs(out['cost'][0].item() - V.COSTS['point']) <= 1e-5 and out['cost'][1].item() <= 1e-6
