"""GPU parity: collision avoidance on every aircraft pair of the multi-aircraft collocation problem (d2d_nlp_solve_groups_pairs,
csrc/nlp_kernels.hip nlp_groups_pairs_kernel) against
  * the CPU statement tests/nlp_groups_pairs_ref.py of the SAME alternation, in constant wind and in a shear, a vortex and a gust,
  * d2d_nlp_solve_groups / d2d_nlp_solve_groups_wind with the masks of the pair (0, 1), bit for bit,
  * the fixed-point certificate (each coupled aircraft re-solved on the CPU against the GPU's partners stays put),
and the planners, the mission chain and the fit backend on top of it.  The tolerances are those tests/test_gpu_mission_wind.py
holds this kernel family to."""
import numpy as np
import pytest

import nlp_groups_pairs_ref as P
import nlp_groups_wind_ref as G
import nlp_wind_ref as R

pytestmark = pytest.mark.gpu
N_AC, N, H = P.N_AC, P.N_NODES, P.H
WINDS = ['const', 'shear', 'vortex', 'gust']


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return R.fields()


def _launch(ctx, rows, W0, field=None, t_start=None, n_ac=N_AC, h=H, max_sweeps=P.MAX_SWEEPS, entry='pairs', **kw):
    """rows (B, SCEN_STRIDE), W0 (B, 5, N) -> W (B, 5, N) and the outputs as numpy."""
    W = ctx.dev(np.ascontiguousarray(W0))
    dsc = ctx.dev(np.ascontiguousarray(rows))
    t = None if field is None else ctx.dev(np.ascontiguousarray(np.asarray(t_start, dtype=np.float64)))
    if entry == 'pairs':
        out = ctx.nlp_solve_groups_pairs(dsc, W, h, n_ac, field, t, max_sweeps=max_sweeps, **kw)
    elif field is None:
        out = ctx.nlp_solve_groups(dsc, W, h, n_ac, max_sweeps=max_sweeps, **kw)
    else:
        out = ctx.nlp_solve_groups_wind(dsc, W, h, n_ac, field, t, max_sweeps=max_sweeps, **kw)
    ctx.sync()
    return W.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if k not in ('work', 't_start') and v is not None}


def _batch(scs):
    return np.concatenate(scs), np.stack([w.T for sc in scs for w in P.guesses(sc)])


def _wind(fields, name):
    return (None, None) if name == 'const' else (fields[name], P.T_STARTS[name])


def _inner(fields, name, r):
    return P.in_constant_wind() if name == 'const' else P.in_field(fields[name], P.T_STARTS[name][r])


@pytest.mark.parametrize('name', WINDS)
def test_all_pairs_against_the_cpu_statement(ctx, fields, name):
    """1. The three crossing scenarios with all six pairs coupled, one launch: statuses and sweep counts equal the statement's, every
    aircraft converged with feas <= 1e-8, cost within 1e-7 relative and nodes within 1e-4 of the statement."""
    scs = P.pair_scenarios()
    rows, W0 = _batch(scs)
    F, ts = _wind(fields, name)
    W, out = _launch(ctx, rows, W0, F, ts)
    for r, sc in enumerate(scs):
        Ws, infos, sweeps, moved = P.solve_groups(P.problems_of(sc), P.guesses(sc), _inner(fields, name, r), P.masks_of(sc), max_sweeps=P.MAX_SWEEPS)
        print(f'{name} scenario {r}: sweeps {out["sweeps"][r]} / {sweeps}, moved {out["moved"][r]:.2e} / {moved:.2e}')
        for a in range(N_AC):
            b = N_AC * r + a
            print(f'  aircraft {a}: status {out["status"][b]} / {infos[a]["status"]}, cost rel {abs(out["cost"][b] - infos[a]["cost"]) / max(infos[a]["cost"], 1e-3):.2e}, '
                  f'nodes {np.abs(W[b].T - Ws[a]).max():.2e}, feas {out["feas"][b]:.2e}, steps {out["iters"][b]} / {infos[a]["inner"]}')
        assert out['sweeps'][r] == sweeps and sweeps <= P.MAX_SWEEPS - 2
        for a in range(N_AC):
            b = N_AC * r + a
            assert out['status'][b] == infos[a]['status'] == 1
            assert out['feas'][b] <= 1e-8
            assert abs(infos[a]['cost'] - out['cost'][b]) <= 1e-7 * max(infos[a]['cost'], 1e-3)
            assert np.abs(W[b].T - Ws[a]).max() <= 1e-4


@pytest.mark.parametrize('name', ['const', 'gust'])
def test_the_default_pair_is_bitwise_the_pair_kernels(ctx, fields, name):
    """2. group_scenarios() with the masks 0b10, 0b01: the new entry point against d2d_nlp_solve_groups (constant wind) and
    d2d_nlp_solve_groups_wind (the gust, a start time per scenario) -- W, cost, feas, iters, status, sweeps, moved array_equal."""
    import d2dhip as D
    scs = G.group_scenarios()
    rows, W0 = _batch(scs)
    rows[0::N_AC, D.SC_PMASK], rows[1::N_AC, D.SC_PMASK] = 0b10, 0b01
    F, ts = (None, None) if name == 'const' else (fields[name], G.T_STARTS[name])
    Wn, on = _launch(ctx, rows, W0, F, ts, max_sweeps=12)
    Wo, oo = _launch(ctx, rows, W0, F, ts, max_sweeps=12, entry='groups')
    assert (oo['sweeps'] >= 1).all()
    assert np.array_equal(Wn, Wo)
    for k in ('cost', 'feas', 'iters', 'status', 'sweeps', 'moved'):
        assert np.array_equal(on[k], oo[k]), k


def test_batches_and_repeats_are_bitwise(ctx, fields):
    """3. R scenarios in one launch equal R single-scenario launches bitwise; two identical launches are bitwise equal."""
    scs = P.pair_scenarios()
    rows, W0 = _batch(scs)
    for name in ('const', 'gust'):
        F, ts = _wind(fields, name)
        W, out = _launch(ctx, rows, W0, F, ts)
        W2, out2 = _launch(ctx, rows, W0, F, ts)
        assert np.array_equal(W, W2) and all(np.array_equal(out[k], out2[k]) for k in ('cost', 'feas', 'iters', 'status', 'sweeps', 'moved'))
        for r in range(len(scs)):
            s = slice(N_AC * r, N_AC * r + N_AC)
            W1, o1 = _launch(ctx, rows[s], W0[s], F, None if ts is None else ts[r:r + 1])
            assert np.array_equal(W1, W[s]) and np.array_equal(o1['cost'], out['cost'][s]) and np.array_equal(o1['iters'], out['iters'][s])
            assert o1['sweeps'][0] == out['sweeps'][r]


@pytest.mark.parametrize('name', WINDS)
def test_fixed_point_certificate(ctx, fields, name):
    """4. Every aircraft of the GPU's answer is a KKT point of its sub-problem against the GPU's positions of ALL its partners (=
    joint KKT): the CPU solver, started there, moves the nodes by <= 1e-5."""
    scs = P.pair_scenarios()
    rows, W0 = _batch(scs)
    F, ts = _wind(fields, name)
    W, out = _launch(ctx, rows, W0, F, ts)
    for r, sc in enumerate(scs):
        pbs = P.problems_of(sc)
        for a in range(N_AC):
            partners = [W[N_AC * r + j, :2].T.copy() for j in P.bits(P.masks_of(sc)[a])]
            Wo, info = P.resolve_one(pbs[a], W[N_AC * r + a].T.copy(), partners, _inner(fields, name, r), a)
            d = np.abs(Wo - W[N_AC * r + a].T).max()
            print(f'{name} scenario {r} aircraft {a}: restart moved the nodes by {d:.2e}')
            assert info['status'] == 1 and d <= 1e-5


def test_all_pairs_keep_the_other_pairs_further_apart(ctx):
    """5. The crossing scenarios in their constant wind: every pair other than (0, 1) that is inside rcol under the default pair is
    further apart under 'all' (strictly; tests/test_collision_pairs_cpu.py checks the same ordering on the CPU)."""
    rows_a, W0 = _batch(P.pair_scenarios())
    rows_d, _ = _batch(P.pair_scenarios([(0, 1)]))
    Wa, oa = _launch(ctx, rows_a, W0)
    Wd, od = _launch(ctx, rows_d, W0)
    Wd2, od2 = _launch(ctx, rows_d, W0, entry='groups')
    assert np.array_equal(Wd, Wd2)
    assert (oa['status'] == 1).all() and (od['status'] == 1).all()
    for r in range(3):
        s = slice(N_AC * r, N_AC * r + N_AC)
        sa = P.min_separation([w.T for w in Wa[s]], P.all_pairs(N_AC)); sd = P.min_separation([w.T for w in Wd[s]], P.all_pairs(N_AC))
        near = [p for p in P.all_pairs(N_AC) if p != (0, 1) and sd[p] < P.RCOL]
        print(r, {p: (round(sd[p], 4), round(sa[p], 4)) for p in near})
        assert len(near) >= 2 and all(sa[p] > sd[p] for p in near)


def _trap(col_pairs, sc, wind=P.CONST_WIND):
    """trap_4 with the end poses of the crossing scenario `sc` (rows) and the collision pairs col_pairs."""
    import d2dhip as D
    import d2d.multiopty_utils as d2mou
    import d2d.opty_utils as d2ou
    import multi_opt_planner as mop

    class S(mop.trap_4):
        pass
    S.cost = d2mou.CostComposit(kvel=70., kbank=1., kobs=float('NaN'), kcol=10., vsp=12, obss=[], obs_kind=0, rcol=10, col_pairs=col_pairs)
    S.t1 = (N - 1) * H
    S.p0s = tuple(tuple(r[D.SC_X0:D.SC_X0 + 3]) + (0., 12.) for r in sc)
    S.p1s = tuple(tuple(r[D.SC_X1:D.SC_X1 + 3]) + (0., 12.) for r in sc)
    S.wind = d2ou.WindField(list(wind))
    return S


def test_planner_plans_with_all_pairs(ctx):
    """6a. multi_opt_planner.Planner(backend='nlp') on a trap_4-like crossing scenario with col_pairs='all': converged,
    info['min_separation'] has the six pairs, and the plan is the direct launch on the Problem's rows."""
    import multi_opt_planner as mop
    sc = P.pair_scenarios()[0]
    p = mop.Planner(_trap('all', sc), backend='nlp')
    rows, coupled = p.prob._rows()
    import d2dhip as D
    cols = [D.SC_X0, D.SC_Y0, D.SC_PSI0, D.SC_X1, D.SC_Y1, D.SC_PSI1, D.SC_S, D.SC_KV, D.SC_KPHI, D.SC_VSP, D.SC_WX, D.SC_WY, D.SC_KCOL, D.SC_RCOL, D.SC_SCOL, D.SC_PMASK]
    assert coupled and np.array_equal(rows[:, cols], sc[:, cols])
    p.prob.addOption('max_sweeps', P.MAX_SWEEPS)
    p.run(tol=1e-7)                       # (the tolerances the scenario was chosen under: opt 1e-7, feas 1e-9)
    assert p.info['status'] == [1, 1, 1, 1] and p.info['status_msg'] == 'converged' and 1 <= p.info['sweeps'] <= P.MAX_SWEEPS - 2
    assert sorted(p.info['min_separation']) == P.all_pairs(N_AC) and len(p.info['min_separation']) == 6
    p.interpret_solution()
    x0 = p.get_initial_guess('tri')
    W0 = np.stack([np.stack([x0[s[a]] for s in (p._slice_x, p._slice_y, p._slice_psi, p._slice_phi, p._slice_v)]) for a in range(N_AC)])
    W, out = _launch(ctx, rows, W0, opt_tol=1e-7, feas_tol=1e-9, inner_max=20, outer_max=36)
    assert np.array_equal(np.stack(p.sol_x), W[:, 0]) and np.array_equal(np.stack(p.sol_y), W[:, 1])
    assert p.info['min_separation'] == pytest.approx(P.min_separation([w.T for w in W], P.all_pairs(N_AC)))
    # the default cost stays on d2d_nlp_solve_groups: one pair reported
    p0 = mop.Planner(_trap(None, sc), backend='nlp')
    p0.prob.addOption('max_sweeps', P.MAX_SWEEPS)
    p0.run(tol=1e-7)
    assert list(p0.info['min_separation']) == [(0, 1)] and p0.prob._pairs is None


@pytest.mark.parametrize('field', [False, True])
def test_mission_plans_through_the_pairs_entry_point(ctx, field):
    """6b. full_sim_phases_batch with col_pairs='all', with and without a wind field: the plan is d2d_nlp_solve_groups_pairs on the
    chain's own rows from the chain's own guess (bitwise), phases 2 and 3 run; with the default cost the chain's output is what the
    existing path (d2d_nlp_solve_groups_wind on the same rows / the fit alone) gives, torch.equal."""
    import torch
    import d2dhip
    import d2d.multiopty_utils as d2mou
    import full_sim as fs
    import multi_opt_planner as mop
    n_ac, c, X1_f, X2_f, X0B, ref3 = G.mission_inputs()
    cB = np.stack([c, c, c])
    F = G.mission_field() if field else None

    class S(mop.trap_4):
        pass
    kw = dict(kvel=70., kbank=1., kobs=float('NaN'), kcol=10., vsp=12, obss=[], obs_kind=0, rcol=10)
    ph1 = fs.CircularFormationGVF_batch(cB, 60, 15, n_ac, X0f=np.stack([X1_f] * 3)[:, :, :3], X0=X0B, record=(), windfield=F)
    t_end = G.mission_t_end(ph1['stop_row'].cpu().numpy(), len(ph1['time']), 0.05, 6, ref3[0], 1)
    run = lambda: fs.full_sim_phases_batch(cB, 60, 15, n_ac, X1_f, S, X2_f, 6, ref3=ref3, t_sim_end=t_end, X0=X0B, windfield=F)      # noqa: E731
    S.cost = d2mou.CostComposit(col_pairs='all', **kw)
    out = run()
    pl = out['plan']
    dctx = d2dhip.default_context()
    dctx.sync()
    assert pl['pairs'] == P.all_pairs(n_ac)
    assert pl['scen'][:, d2dhip.SC_PMASK].cpu().numpy().reshape(3, n_ac).tolist() == [[0b1110, 0b1101, 0b1011, 0b0111]] * 3
    # (the fit plan is cached: the chain's guess is its q sampled again)
    N2, dt2, dur2 = mop.d2ou.planner_timing(S.t0, S.t1, S.hz)
    plan = mop.sop.get_plan(N2, dur2, S.obj_scale / N2 / n_ac, 70., 1.)
    _, Xs = plan.sample(pl['scen'], pl['q'])
    Wd = Xs.contiguous().clone()
    direct = dctx.nlp_solve_groups_pairs(pl['scen'], Wd, float(dt2), n_ac, pl.get('field'), pl.get('t_start'))
    dctx.sync()
    assert torch.equal(Wd, pl['W']) and torch.equal(direct['cost'], pl['cost']) and torch.equal(direct['sweeps'], pl['sweeps'])
    print('status', pl['status'].cpu().numpy(), 'sweeps', pl['sweeps'].cpu().numpy(), 'moved', pl['moved'].cpu().numpy())
    assert float(pl['feas'].max().item()) <= 1e-8 and bool((pl['status'] != 3).all().item())
    assert torch.isfinite(out['phase2']['X_final']).all() and len(out['phase3']) >= 1 and torch.isfinite(out['phase3'][-1]['X_final']).all()
    # the default cost: the chain as it was
    S.cost = d2mou.CostComposit(**kw)
    out0 = run()
    pl0 = out0['plan']
    assert 'pairs' not in pl0
    if field:
        W0 = plan.sample(pl0['scen'], pl0['q'])[1].contiguous().clone()
        old = dctx.nlp_solve_groups_wind(pl0['scen'], W0, float(dt2), n_ac, pl0['field'], pl0['t_start'])
        dctx.sync()
        assert torch.equal(W0, pl0['W']) and torch.equal(old['cost'], pl0['cost'])
    else:
        assert 'W' not in pl0 and torch.equal(pl0['Xs'], plan.sample(pl0['scen'], pl0['q'])[1])
    out1 = run()
    assert torch.equal(out0['phase2']['X_final'], out1['phase2']['X_final']) and torch.equal(out0['plan']['Xs'], out1['plan']['Xs'])


def test_malformed_masks_refuse_their_scenario_only(ctx):
    """7. A scenario whose masks are malformed -- a bit at or above n_ac, a self bit, a bit the partner does not return, no integer --
    is refused on the device: D2D_ST_NONFINITE, cost = feas = NaN, sweeps = 0, its W untouched; the other scenarios of the launch
    are solved as if alone.  f without t_start is D2D_EINVAL before anything is launched."""
    import d2dhip as D
    scs = P.pair_scenarios()
    good, W0g = _batch(scs[:1])
    Wg, og = _launch(ctx, good, W0g)
    bads = []
    for col, val in ((0, 0b10000 | 0b1110), (1, 0b1111), (3, 2.5), (0, -2.0), (1, float('nan')), (2, 256.0 + 0b1011)):
        b = scs[1].copy()
        b[col, D.SC_PMASK] = val
        bads.append(b)
    asym = scs[1].copy(); asym[0, D.SC_PMASK] = 0b0110                 # aircraft 3 still names aircraft 0
    bads.append(asym)
    for b in bads:
        rows = np.concatenate([b, good]); W0 = np.concatenate([_batch([b])[1], W0g])
        W, out = _launch(ctx, rows, W0)
        assert (out['status'][:N_AC] == D.ST_NONFINITE).all() and np.isnan(out['cost'][:N_AC]).all() and np.isnan(out['feas'][:N_AC]).all()
        assert out['sweeps'][0] == 0 and out['moved'][0] == 0.0 and (out['iters'][:N_AC] == 0).all()
        assert np.array_equal(W[:N_AC], W0[:N_AC])
        assert np.array_equal(W[N_AC:], Wg) and np.array_equal(out['cost'][N_AC:], og['cost']) and out['sweeps'][1] == og['sweeps'][0]
    import ctypes as C
    W = ctx.dev(W0g.copy())
    o = D.NlpOpts(10.0, 0.1, 1e-9, 1e-9, 1e-7, 20, 120, 0, 0, None, None)
    f = D._wind_c(ctx, R.fields()['shear'])
    work = ctx.empty((ctx.lib.d2d_nlp_workspace_doubles(N) * N_AC + 2 * N) * 1)
    cost, feas = ctx.empty(N_AC), ctx.empty(N_AC)
    rc = ctx.lib.d2d_nlp_solve_groups_pairs(ctx.h, 1, N_AC, N, H, D._ptr(ctx.dev(good)), C.byref(o), 12, 1e-7, D._ptr(W), D._ptr(work), None,
                                            D._ptr(cost), D._ptr(feas), None, None, None, None, C.byref(f), None)
    ctx.sync()
    assert rc == -1 and np.array_equal(W.cpu().numpy(), W0g)              # D2D_EINVAL: a field without start times


def test_fit_backend_couples_the_selected_pairs():
    """8. backend='fit' gets the pairs through SC_PMASK: plan.solve_groups on the rows multi_opt_planner.scenario_rows lowers for
    col_pairs='all' (four aircraft to their antipodes on a circle, d2dhip.synth.circle_group_scenarios) against oracle/fit.py's
    bgs_solve, to the tolerance of tests/test_gpu_groups.py (1e-6 relative on the polynomial coefficients and on the joint cost)."""
    import d2dhip as D
    from d2dhip import synth
    from oracle import fit as F
    import d2d.multiopty_utils as d2mou
    import multi_opt_planner as mop
    K = 50
    dur = F.planner_timing(0, 4.9, 10)[2]
    base = synth.circle_group_scenarios(4, 1, dur, K, seed=4, obj_scale=1.0)[0]

    class S(mop.exp_5):
        pass
    S.hz, S.t1, S.vref, S.obj_scale = 10, 4.9, 12, 1.0
    S.cost = d2mou.CostComposit(kvel=5., kbank=1., kobs=float('NaN'), kcol=10., vsp=12, obss=[], obs_kind=0, rcol=10, col_pairs='all')
    S.p0s = tuple(tuple(r[D.SC_X0:D.SC_X0 + 3]) + (0., 12.) for r in base)
    S.p1s = tuple(tuple(r[D.SC_X1:D.SC_X1 + 3]) + (0., 12.) for r in base)
    rows, plan, coupled = mop.scenario_rows(S, S.p0s, S.p1s, K, dur, S.obj_scale, (0., 0.))
    assert coupled and rows[:, D.SC_PMASK].tolist() == [0b1110, 0b1101, 0b1011, 0b0111]
    ctx = D.default_context()
    ob = F.FitBasis.from_arrays(mop.sop.N_SEG, K, dur, *plan.basis())
    dsc = ctx.dev(rows)
    q = plan.init(dsc)
    try:
        cost, sweeps, stats = plan.solve_groups(dsc, q, 4, max_sweeps=80, inner_iters=8, tol=1e-12)
    finally:
        plan.set_groups(1)
    assert sweeps < 80, (sweeps, stats)
    qh = q.cpu().numpy()
    qo, co, swo = F.bgs_solve(ob, rows, sweeps=80, inner_iters=8, tol=1e-12, ls=True)
    zg = np.array([F.coefficients(ob, rows[i], qh[i]) for i in range(4)]); zo = np.array([F.coefficients(ob, rows[i], qo[i]) for i in range(4)])
    cj = F.group_cost(ob, rows, qh)
    print('sweeps', sweeps, swo, 'coefficients rel', np.abs(zg - zo).max() / np.abs(zo).max(), 'cost rel', abs(co - cj) / cj)
    assert np.abs(zg - zo).max() <= 1e-6 * np.abs(zo).max()
    assert abs(co - cj) <= 1e-6 * cj
    # and the planner reports the six separations
    p = mop.Planner(S, backend='fit')
    p.run()
    assert sorted(p.info['min_separation']) == P.all_pairs(4)
