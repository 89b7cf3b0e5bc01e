"""GPU parity: collocation plans around moving obstacles (d2d_mov_sample, d2d_nlp_solve_moving, d2d_nlp_solve_groups_moving;
csrc/nlp_kernels.hip nlp_mov_sample_kernel and the MOV instantiations) against
  * the CPU statement tests/nlp_moving_ref.py, single problems and groups, in constant wind and in the unsteady gust,
  * the entries without moving obstacles (d2d_nlp_solve, d2d_nlp_solve_wind, d2d_nlp_solve_groups_pairs), bit for bit when nothing moves,
  * the static disc of the scenario row when the track stands still,
and the refusals, the planner and the mission chain on top.  Tolerances: those tests/test_gpu_mission_wind.py and
tests/test_gpu_collision_pairs.py hold this kernel family to -- status equal, feas <= 1e-8, cost within 1e-7 relative, nodes within 1e-4."""
import numpy as np
import pytest

import nlp_groups_pairs_ref as P
import nlp_moving_ref as M
import nlp_wind_ref as R
from d2d.opty_utils import MovingObstacle

pytestmark = pytest.mark.gpu
N, H = M.N_NODES, M.H
OUT = ('cost', 'feas', 'iters', 'status')


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
    return {k: v.cpu().numpy() for k, v in out.items() if k not in ('work', 't_start') and v is not None}


def _run(ctx, fn, *a, **kw):
    out = fn(*a, **kw)
    ctx.sync()
    return _np(out)


def _solve(ctx, rows, W0, moving=None, field=None, t_start=None, h=H, tabs=None):
    """rows (B, SCEN_STRIDE), W0 (B, 5, N), moving: one disc list per problem -> W (B, 5, N) and the outputs as numpy."""
    W = ctx.dev(np.ascontiguousarray(W0)); dsc = ctx.dev(np.ascontiguousarray(rows))
    kn, dc = tabs if tabs is not None else (M.tables(moving) if moving is not None else (None, None))
    t = None if t_start is None else ctx.dev(np.ascontiguousarray(np.asarray(t_start, dtype=np.float64)))
    out = ctx.nlp_solve_moving(dsc, W, h, None if kn is None else ctx.dev(kn), None if dc is None else ctx.dev(dc), field, t)
    ctx.sync()
    return W.cpu().numpy(), _np(out)


def _groups(ctx, rows, W0, moving=None, field=None, t_start=None, n_ac=P.N_AC, tabs=None, max_sweeps=P.MAX_SWEEPS):
    W = ctx.dev(np.ascontiguousarray(W0)); dsc = ctx.dev(np.ascontiguousarray(rows))
    kn, dc = tabs if tabs is not None else (M.tables(moving) if moving is not None else (None, None))
    t = None if t_start is None else ctx.dev(np.ascontiguousarray(np.asarray(t_start, dtype=np.float64)))
    out = ctx.nlp_solve_groups_moving(dsc, W, H, n_ac, None if kn is None else ctx.dev(kn), None if dc is None else ctx.dev(dc), field, t,
                                      max_sweeps=max_sweeps)
    ctx.sync()
    return W.cpu().numpy(), _np(out)


def _check(tag, W, out, b, Wo, info):
    rel = abs(out['cost'][b] - info['cost']) / max(info['cost'], 1e-3)
    dn = np.abs(W[b].T - Wo).max()
    print(f'{tag}: status {out["status"][b]} / {info["status"]}, cost rel {rel:.2e}, nodes {dn:.2e}, feas {out["feas"][b]:.2e}, '
          f'steps {out["iters"][b]} / {info["inner"]}')
    assert out['status'][b] == info['status'] == 1
    assert out['feas'][b] <= 1e-8
    assert rel <= 1e-7
    assert dn <= 1e-4


@pytest.mark.parametrize('n_knot', [2, 5])
@pytest.mark.parametrize('n_nodes', [61, 121])
def test_sampler_against_the_numpy_twin(ctx, n_knot, n_nodes):
    """1. d2d_mov_sample against MovingObstacle.at: three discs, two problems with different start times, the first node before the
    first knot and the last nodes after the last knot; coordinates of order 1e2, difference <= 1e-12 (a few ulps of one multiply-add
    and one division; measured: see DESIGN.md 5.13)."""
    rng = np.random.default_rng(n_knot)
    t_starts = np.array([1.75, 40.5])
    discs = []
    for g in range(2):
        tk = t_starts[g] + 0.33 + np.sort(rng.uniform(0.0, 0.6 * (n_nodes - 1) * H, n_knot))
        tk += 1e-3 * np.arange(n_knot)
        discs.append([MovingObstacle(tk, rng.uniform(-150.0, 150.0, (n_knot, 2)), 5.0 + m, kind=m % 2) for m in range(3)])
    kn, dc = M.tables(discs)
    ctr = ctx.mov_sample(ctx.dev(kn), ctx.dev(dc), ctx.dev(t_starts), n_nodes, H).cpu().numpy()
    assert ctr.shape == (2, 3, 2, n_nodes)
    worst = 0.0
    for g in range(2):
        t = M.node_times(t_starts[g], n_nodes)
        assert t[0] < discs[g][0].t[0] and t[-1] > discs[g][0].t[-1]
        for m, o in enumerate(discs[g]):
            ref = o.at(t)
            worst = max(worst, np.abs(ctr[g, m].T - ref).max())
            assert np.array_equal(ctr[g, m, :, 0], o.xy[0]) and np.array_equal(ctr[g, m, :, -1], o.xy[-1])      # held outside the knots
    print(f'sampler N = {n_nodes}, n_knot = {n_knot}: max |device - numpy| = {worst:.2e}')
    assert worst <= 1e-12


@pytest.mark.parametrize('wind', ['const', 'gust'])
@pytest.mark.parametrize('kind', [1, 0])
def test_catalogue_against_the_cpu_statement(ctx, fields, wind, kind):
    """2. The three starting scenarios of one kind in one launch, in still air and in the unsteady gust from t_start = 2.5 s."""
    cases = [c for c in M.cases() if c[0] == wind and c[1] == kind]
    F = None if wind == 'const' else fields['gust']
    rows = np.stack([M.row(kind, p1=(leg, 0.0, 0.0)) for _, _, _, leg, _ in cases])
    mv = [M.catalogue(kind, t0, leg)[name] + ([MovingObstacle.linear((0, 0), (0, 0), -1.0)] if name != 'two' else [])
          for _, _, name, leg, t0 in cases]                 # (one table shape per call: the one-disc scenarios carry an absent second disc)
    W0 = np.stack([M.straight_guess(r).T for r in rows])
    ts = [c[4] for c in cases]
    W, out = _solve(ctx, rows, W0, mv, F, ts)
    for b, (_, _, name, leg, t0) in enumerate(cases):
        Wo, info = M.solve(M.problem(rows[b], mv[b], t0), W0[b].T, F, t0)
        _check(f'{wind} kind {kind} {name}', W, out, b, Wo, info)
        assert np.abs(Wo[:, 1]).max() > 3.0                 # the plan goes round the disc


def test_one_hundred_and_twenty_one_nodes(ctx):
    """2b. exp_14's shape: a wave of 64 lanes walks 121 nodes in two passes.  The crossing of the catalogue on a 12 s leg."""
    n = 121
    r = M.row(1, p1=(144.0, 0.0, 0.0), N=n)
    mv = [MovingObstacle.linear((72.0, -56.0), (0.0, 10.0), 8.0, t0=1.0, t1=21.0)]
    W0 = M.straight_guess(r, n)
    W, out = _solve(ctx, r[None], W0.T[None], [mv], None, [1.0])
    Wo, info = M.solve(M.problem(r, mv, 1.0, N=n), W0)
    _check('N = 121 crossing', W, out, 0, Wo, info)
    assert np.abs(Wo[:, 1]).max() > 3.0


def test_nothing_moving_is_bitwise_the_old_single_entries(ctx, fields):
    """3a. n_mov = 0 and every r <= 0: W, cost, feas, iters, status equal d2d_nlp_solve (constant wind) and d2d_nlp_solve_wind (the
    gust, all start times equal) bit for bit.  The rows carry a static disc, so the exp terms are exercised."""
    import d2dhip as D
    rows = np.stack([M.row(1), M.row(0), M.row(1, p1=(70.0, 4.0, 0.1))])
    rows[:, D.SC_O0X:D.SC_O0X + 3] = (36.0, 1.0, 6.0); rows[1, D.SC_OKIND] = 1
    W0 = np.stack([M.straight_guess(r).T for r in rows])
    absent = [[MovingObstacle.linear((30, 0), (1, 1), 0.0), MovingObstacle.linear((40, 0), (1, 1), -2.0, kind=0)]] * 3
    dsc = ctx.dev(rows)
    Wa = ctx.dev(W0.copy()); oa = _run(ctx, ctx.nlp_solve, dsc, Wa, H)
    assert (oa['status'] == 1).all()
    for mv, ts in ((None, None), (absent, [3.0] * 3)):
        W, out = _solve(ctx, rows, W0, mv, None, ts)
        assert np.array_equal(W, Wa.cpu().numpy()) and all(np.array_equal(out[k], oa[k]) for k in OUT)
    rows_g = np.stack([M.row(1, p1=(M.LEG_GUST, 0.0, 0.0)), M.row(0, p1=(M.LEG_GUST, 2.0, 0.0))])
    rows_g[:, D.SC_O0X:D.SC_O0X + 3] = (24.0, 1.0, 5.0); rows_g[1, D.SC_OKIND] = 1
    W0g = np.stack([M.straight_guess(r).T for r in rows_g])
    Wb = ctx.dev(W0g.copy()); ob = _run(ctx, ctx.nlp_solve_wind, ctx.dev(rows_g), Wb, H, fields['gust'], t_start=2.5)
    assert (ob['status'] == 1).all()
    for mv in (None, absent[:2]):
        W, out = _solve(ctx, rows_g, W0g, mv, fields['gust'], [2.5, 2.5])
        assert np.array_equal(W, Wb.cpu().numpy()) and all(np.array_equal(out[k], ob[k]) for k in OUT)


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_nothing_moving_is_bitwise_the_pairs_entry(ctx, fields, wind):
    """3b. Groups: n_mov = 0 and r <= 0 against d2d_nlp_solve_groups_pairs -- W, cost, feas, iters, status, sweeps, moved."""
    scs = P.pair_scenarios()[:2]
    rows = np.concatenate(scs); W0 = np.stack([w.T for sc in scs for w in P.guesses(sc)])
    F, ts = (None, None) if wind == 'const' else (fields['gust'], list(P.T_STARTS['gust'][:2]))
    Wo = ctx.dev(W0.copy())
    oo = _run(ctx, ctx.nlp_solve_groups_pairs, ctx.dev(rows), Wo, H, P.N_AC, F, None if ts is None else ctx.dev(np.array(ts)), max_sweeps=P.MAX_SWEEPS)
    assert (oo['sweeps'] >= 1).all()
    absent = [[MovingObstacle.linear((-13, 0), (1, 1), 0.0)]] * 2
    for mv, t in ((None, ts), (absent, ts if ts is not None else [0.0, 0.0])):
        W, out = _groups(ctx, rows, W0, mv, F, t)
        assert np.array_equal(W, Wo.cpu().numpy())
        for k in OUT + ('sweeps', 'moved'):
            assert np.array_equal(out[k], oo[k]), k


@pytest.mark.parametrize('kind', [1, 0])
def test_a_track_that_stands_still_is_the_static_disc(ctx, kind):
    """4. One disc with both knots at the same place against the same disc in the scenario row, the only exp term either way: the
    family tolerances (the sums are the same expressions on the same centres; the difference is printed and noted in DESIGN.md 5.13)."""
    import d2dhip as D
    r_mov = M.row(kind); r_sta = r_mov.copy()
    r_sta[D.SC_O0X:D.SC_O0X + 3] = (36.0, 1.5, 8.0); r_sta[D.SC_OKIND] = 1 if kind == 0 else 0
    W0 = M.straight_guess(r_mov).T[None]
    Ws = ctx.dev(W0.copy()); os_ = _run(ctx, ctx.nlp_solve, ctx.dev(r_sta[None]), Ws, H)
    W, out = _solve(ctx, r_mov[None], W0, [[MovingObstacle((0.0, 10.0), ((36.0, 1.5), (36.0, 1.5)), 8.0, kind=kind)]], None, [2.0])
    dn = np.abs(W - Ws.cpu().numpy()).max(); rel = abs(out['cost'][0] - os_['cost'][0]) / os_['cost'][0]
    print(f'stand-still kind {kind}: nodes differ by {dn:.2e}, cost rel {rel:.2e}, steps {out["iters"][0]} / {os_["iters"][0]}')
    assert out['status'][0] == os_['status'][0] == 1 and out['feas'][0] <= 1e-8
    assert rel <= 1e-7 and dn <= 1e-4


def test_batches_and_repeats_are_bitwise(ctx, fields):
    """5. A batch equals its single launches bitwise; two identical launches are bitwise equal (single problems in the gust, groups
    in constant wind)."""
    cases = [c for c in M.cases() if c[0] == 'gust' and c[1] == 1]
    rows = np.stack([M.row(1, p1=(leg, 0.0, 0.0)) for _, _, _, leg, _ in cases])
    mv = [M.catalogue(1, t0, leg)['two'] for _, _, _, leg, t0 in cases]
    W0 = np.stack([M.straight_guess(r).T for r in rows]); ts = [c[4] + 0.5 * b for b, c in enumerate(cases)]
    W, out = _solve(ctx, rows, W0, mv, fields['gust'], ts)
    W2, out2 = _solve(ctx, rows, W0, mv, fields['gust'], ts)
    assert np.array_equal(W, W2) and all(np.array_equal(out[k], out2[k]) for k in OUT)
    for b in range(len(cases)):
        W1, o1 = _solve(ctx, rows[b:b + 1], W0[b:b + 1], mv[b:b + 1], fields['gust'], ts[b:b + 1])
        assert np.array_equal(W1[0], W[b]) and all(np.array_equal(o1[k][0], out[k][b]) for k in OUT)
    scs = M.group_scenarios(); discs = M.group_discs()
    rg = np.concatenate(scs); Wg0 = np.stack([w.T for sc in scs for w in P.guesses(sc)])
    Wg, og = _groups(ctx, rg, Wg0, discs, None, [0.0, 0.0])
    Wg2, og2 = _groups(ctx, rg, Wg0, discs, None, [0.0, 0.0])
    assert np.array_equal(Wg, Wg2) and all(np.array_equal(og[k], og2[k]) for k in OUT + ('sweeps', 'moved'))
    for r in range(2):
        s = slice(P.N_AC * r, P.N_AC * (r + 1))
        W1, o1 = _groups(ctx, rg[s], Wg0[s], discs[r:r + 1], None, [0.0])
        assert np.array_equal(W1, Wg[s]) and np.array_equal(o1['cost'], og['cost'][s]) and o1['sweeps'][0] == og['sweeps'][r]


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_fewer_slots_than_problems_and_the_order_only_schedule(ctx, fields, wind):
    """5b. The hand-out loop of the moving kernels: six problems of 41 nodes by the catalogue's rule (4 s legs: 48 m in still air, 32 m
    in the gust), problem 3's track with times that do not increase.  (a) index order, default slots; (b) two slots and the reversed
    order: a slot takes a third ticket, the refused problem lies between two solved ones -- W, cost, feas, iters, status equal (a)
    bitwise; (c) two slots and the order with problem 1's entry replaced by an index outside [0, B): the others equal (a) bitwise,
    problem 1 keeps its guess (its outputs are not written: compared only where defined).  The refused problem: ST_NONFINITE, NaN cost,
    W bitwise its guess, in every run."""
    import torch
    import d2dhip as D
    n, B, BAD, DROP = 41, 6, 3, 1
    leg, t0, F = (48.0, 0.0, None) if wind == 'const' else (32.0, M.GUST_T_START, fields['gust'])
    kinds, names = (1, 1, 1, 0, 0, 0), ('crossing', 'headon', 'two') * 2
    rows = np.stack([M.row(k, p1=(leg, 0.0, 0.0), N=n) for k in kinds])
    mv = [M.catalogue(k, t0, leg)[nm] + ([MovingObstacle.linear((0, 0), (0, 0), -1.0)] if nm != 'two' else []) for k, nm in zip(kinds, names)]
    kn, dc = M.tables(mv)
    kn[BAD, 0, 1, 0] = kn[BAD, 0, 0, 0]
    W0 = np.stack([M.straight_guess(r, n).T for r in rows])
    dsc, dkn, ddc, dts = ctx.dev(rows), ctx.dev(kn), ctx.dev(dc), ctx.dev(t0 + 0.25 * np.arange(B))

    def run(**kw):
        W = ctx.dev(W0.copy())
        out = ctx.nlp_solve_moving(dsc, W, H, dkn, ddc, F, dts, **kw)
        ctx.sync()
        return W.cpu().numpy(), _np(out)

    def order(perm):
        return torch.from_numpy(np.asarray(perm, dtype=np.int32)).to(ctx.device)

    rev = np.arange(B)[::-1].copy()
    dropped = rev.copy(); dropped[rev == DROP] = B
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


@pytest.mark.parametrize('wind', ['const', 'gust'])
def test_groups_against_the_cpu_statement(ctx, fields, wind):
    """6. Two four-aircraft crossings, all six pairs coupled, one moving disc through each, one launch: statuses and sweep counts
    equal the statement's, every aircraft within the family tolerances."""
    scs = M.group_scenarios()
    ts = [0.0, 0.0] if wind == 'const' else list(P.T_STARTS['gust'][:2])
    discs = M.group_discs(ts)
    F = None if wind == 'const' else fields['gust']
    rows = np.concatenate(scs); W0 = np.stack([w.T for sc in scs for w in P.guesses(sc)])
    W, out = _groups(ctx, rows, W0, discs, F, ts)
    for r, sc in enumerate(scs):
        Ws, infos, sweeps, moved = M.solve_groups(sc, discs[r], P.guesses(sc), F, ts[r])
        print(f'{wind} scenario {r}: sweeps {out["sweeps"][r]} / {sweeps}, moved {out["moved"][r]:.2e} / {moved:.2e}')
        assert out['sweeps'][r] == sweeps and sweeps <= P.MAX_SWEEPS - 2
        for a in range(P.N_AC):
            _check(f'  aircraft {a}', W, out, P.N_AC * r + a, Ws[a], infos[a])


def test_refusals(ctx):
    """7. A launch of three: a NaN knot refuses problem 0, equal knot times problem 1 -- status ST_NONFINITE, cost = feas = NaN,
    iters 0, W untouched -- and problem 2 is solved.  A kind of 2 refuses a whole scenario of a group.  Host errors: D2D_EINVAL."""
    import d2dhip as D
    rows = np.stack([M.row(1)] * 3); W0 = np.stack([M.straight_guess(r).T for r in rows])
    mv = [M.catalogue(1)['crossing']] * 3
    kn, dc = M.tables(mv)
    kn[0, 0, 1, 1] = np.nan; kn[1, 0, 1, 0] = kn[1, 0, 0, 0]
    W, out = _solve(ctx, rows, W0, tabs=(kn, dc), t_start=[0.0] * 3)
    for b in (0, 1):
        assert out['status'][b] == D.ST_NONFINITE and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and out['iters'][b] == 0
        assert np.array_equal(W[b], W0[b])
    Wo, info = M.solve(M.problem(rows[2], mv[2], 0.0), W0[2].T)
    _check('the third problem', W, out, 2, Wo, info)
    scs = M.group_scenarios(); rg = np.concatenate(scs); Wg0 = np.stack([w.T for sc in scs for w in P.guesses(sc)])
    kn, dc = M.tables(M.group_discs()); dc[1, 0, 1] = 2.0
    Wg, og = _groups(ctx, rg, Wg0, tabs=(kn, dc), t_start=[0.0, 0.0])
    s = slice(P.N_AC, 2 * P.N_AC)
    assert (og['status'][s] == D.ST_NONFINITE).all() and np.isnan(og['cost'][s]).all() and (og['iters'][s] == 0).all() and og['sweeps'][1] == 0
    assert np.array_equal(Wg[s], Wg0[s]) and (og['status'][:P.N_AC] == 1).all()
    kn, dc = M.tables(mv)
    dsc, Wd = ctx.dev(rows), ctx.dev(W0.copy())
    with pytest.raises(D.D2DError, match='t_start'):
        ctx.nlp_solve_moving(dsc, Wd, H, ctx.dev(kn), ctx.dev(dc), None, None)
    with pytest.raises(D.D2DError, match='n_mov'):
        ctx.nlp_solve_moving(dsc, Wd, H, ctx.dev(np.repeat(kn, 9, 1)), ctx.dev(np.repeat(dc, 9, 1)), None, 0.0)
    with pytest.raises(D.D2DError, match='n_knot'):
        ctx.nlp_solve_moving(dsc, Wd, H, ctx.dev(np.repeat(kn, 17, 2)), ctx.dev(dc), None, 0.0)
    with pytest.raises(D.D2DError, match='n_knot'):
        ctx.mov_sample(ctx.dev(kn[:, :, :1]), ctx.dev(dc), 0.0, N, H)
    with pytest.raises(D.D2DError, match='go together'):
        ctx.nlp_solve_moving(dsc, Wd, H, None, None, None, 0.0)
    ctx.sync()
    assert np.array_equal(Wd.cpu().numpy(), W0)


def test_planner_routes_to_the_collocation_backend(ctx):
    """8a. Planner(exp) with exp.moving_obstacles: backend_used == 'nlp', min_clearance per disc, the plan equals the statement's."""
    import d2d.opty_utils as d2ou
    import single_opt_planner as sop

    class exp(sop.exp_1):
        t0, t1, hz = 4.0, 10.0, 10
        p0, p1 = (0., 0., 0., 0., 12.), (72., 0., 0., 0., 12.)
        cost, obj_scale = d2ou.CostComposit(kvel=70., kbank=1., kobs=10., vsp=12., obss=[]), 1.
        x_constraint = y_constraint = None
        phi_constraint, v_constraint = (-np.deg2rad(30.), np.deg2rad(30.)), (9., 14.)
        moving_obstacles = M.catalogue(1, 4.0)['two']
    p = sop.Planner(exp)
    p.run(M.straight_guess(M.row(1)).T.reshape(-1))
    assert p.info['backend_used'] == 'nlp' and p.info['status'] == 1
    Wo, info = M.solve(M.problem(M.row(1), exp.moving_obstacles, 4.0), M.straight_guess(M.row(1)))
    assert np.abs(np.stack([p.sol_x, p.sol_y], 1) - Wo[:, :2]).max() <= 1e-4
    tn = M.node_times(4.0)
    ref = [float(np.hypot(*(Wo[:, :2] - o.at(tn)).T).min() - o.r) for o in exp.moving_obstacles]
    print('min_clearance', p.info['min_clearance'], ref)
    assert len(p.info['min_clearance']) == 2 and np.allclose(p.info['min_clearance'], ref, atol=2e-4)
    assert abs(p.info['cost'] - info['cost']) <= 1e-7 * info['cost']


def test_mission_plans_each_formation_from_its_own_time(ctx):
    """8b. full_sim_phases_batch(moving_obstacles=...) with two formations whose phase 1 ends at different times: each transition is
    planned around the disc at its own start time -- the plan equals the statement run from the same end-of-phase-1 states and time
    within the mission test's tolerances (status equal, feas <= 1e-8, cost 1e-7 relative, nodes 1e-4) -- and the two plans differ."""
    import d2dhip as D
    import d2d.multiopty_utils as d2mou
    import full_sim as fs
    import multi_opt_planner as mop
    import nlp_groups_wind_ref as G

    class scen(mop.trap_4):
        cost = d2mou.CostComposit(kvel=70., kbank=1., kobs=10., kcol=10., vsp=12., obss=[], obs_kind=1, rcol=10)
    n_ac, c, X1_f, X2_f, X0B, ref3 = G.mission_inputs()
    cB, X0 = np.stack([c, c]), X0B[:2]
    r, v, t_opt, t_step = 60, 15, 6, 0.05
    ph1 = fs.CircularFormationGVF_batch(cB, r, v, n_ac, X0f=np.stack([X1_f] * 2)[:, :, :3], t_step=t_step, t_end=1000., X0=X0, record=())
    ctx.sync()
    stop = ph1['stop_row'].cpu().numpy()
    t2h = (np.minimum(stop, len(ph1['time'])) - 1) * t_step
    assert stop[0] != stop[1]
    # a disc that climbs through the upper legs (y = 40) at x = 50 about three seconds after the formations start their transitions
    tm = float(t2h.mean()) + 3.0
    disc = [MovingObstacle((tm - 40.0, tm + 40.0), ((50.0, 40.0 - 400.0), (50.0, 40.0 + 400.0)), 8.0)]
    out = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, scen, X2_f, t_opt, ref3=None, X0=X0, moving_obstacles=disc)
    ctx.sync()
    pl = out['plan']
    np.testing.assert_array_equal(pl['t_start'].cpu().numpy(), t2h)
    rows = pl['scen'].cpu().numpy(); W = pl['W'].cpu().numpy(); st = pl['status'].cpu().numpy()
    n_nodes = W.shape[2]; h = t_opt / (n_nodes - 1)
    _, plan, _ = mop.scenario_rows(scen, [(0., 0., 0., 0., 0.)] * n_ac, X2_f, n_nodes, float(t_opt), scen.obj_scale, scen.wind.w)
    Xg = plan.sample(pl['scen'], pl['q'])[1].cpu().numpy()          # the fit's plan: the guess the chain started from
    o = {k: pl[k].cpu().numpy() for k in ('cost', 'feas', 'iters', 'status', 'sweeps', 'moved')}
    print('start times', t2h, 'status', st, 'sweeps', o['sweeps'])
    assert (rows[:, D.SC_KOBS] == 10.0).all()
    for f in range(2):
        s = slice(n_ac * f, n_ac * (f + 1))
        Ws, infos, sweeps, moved = M.solve_groups(rows[s], disc, [Xg[b].T for b in range(s.start, s.stop)], None, t2h[f], max_sweeps=12, N=n_nodes, h=h)
        assert o['sweeps'][f] == sweeps
        for a in range(n_ac):
            _check(f'formation {f} aircraft {a}', W, o, n_ac * f + a, Ws[a], infos[a])
        clr = d2ou_min_clearance(disc, M.node_times(t2h[f], n_nodes, h), W[s])
        print(f'formation {f}: clearance per aircraft {np.round(clr, 2)}')
    # the two formations start from different states at different times: their plans differ, and so do the discs they saw
    assert np.abs(W[:n_ac] - W[n_ac:]).max() > 1e-3
    ctr = pl['mov_work'].cpu().numpy()
    assert np.abs(ctr[0] - ctr[1]).max() >= 10.0 * abs(t2h[0] - t2h[1]) * 0.99


def d2ou_min_clearance(disc, t, Ws):
    from d2d.opty_utils import min_clearance
    return [min_clearance(disc, t, w[0], w[1])[0] for w in Ws]
