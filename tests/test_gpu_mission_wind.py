"""GPU parity: the multi-aircraft collocation problem in a wind field (d2d_nlp_solve_groups_wind, csrc/nlp_kernels.hip
nlp_groups_wind_kernel), tracking from per-drone start times (d2d_sim_track_run_wind_at) and the three-phase mission chained through
a field (full_sim.full_sim_phases_batch(windfield=)), against
  * d2d_nlp_solve_groups in a spatially uniform field, d2d_nlp_solve_wind with one aircraft per scenario,
  * the CPU statement tests/nlp_groups_wind_ref.py (block Gauss-Seidel over tests/nlp_wind_ref.py) in a shear, a vortex and a gust,
  * the joint KKT conditions in the field, and the scalar tracking entry point.
The tolerances are those the existing collocation and tracking tests hold the kernels to."""
import numpy as np
import pytest

import nlp_groups_wind_ref as G
import nlp_wind_ref as R
from oracle import nlp

pytestmark = pytest.mark.gpu
N_AC, N, H = G.N_AC, G.N_NODES, G.H


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return R.fields()


def _launch(ctx, rows, W0, field, t_start, n_ac=N_AC, h=H, **kw):
    """rows (B, SCEN_STRIDE), W0 (B, 5, N), t_start (R,) -> W (B, 5, N) and the outputs as numpy."""
    W = ctx.dev(np.ascontiguousarray(W0))
    t = ctx.dev(np.ascontiguousarray(np.asarray(t_start, dtype=np.float64)))
    out = ctx.nlp_solve_groups_wind(ctx.dev(np.ascontiguousarray(rows)), W, h, n_ac, field, t, **kw)
    ctx.sync()
    return W.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if k != 'work'}


def _batch(no_wind_columns=True):
    import d2dhip as D
    scs = G.group_scenarios()
    rows = np.concatenate(scs)
    W0 = np.stack([w.T for sc in scs for w in G.guesses(sc)])
    if no_wind_columns:
        rows[:, D.SC_WX] = rows[:, D.SC_WY] = np.nan          # not read in a field
    return scs, rows, W0


def _joint_scenarios(gold):
    """The scenarios of tests/test_gpu_nlp.py test_joint_problems_in_batches_equal_the_single_launches: rows (24, .), W0 (24, 5, 71), h."""
    import d2dhip
    import multi_opt_planner as mop
    from test_gpu_nlp import _trap4_like_the_golden
    scen, keep, Wg, g = _trap4_like_the_golden(gold)
    try:
        _p = mop.Planner(scen, initialize=True, backend='nlp')
        rows, coupled = _p.prob._rows()
        assert coupled
        x0 = _p.get_initial_guess('tri')
        W0 = np.stack([np.stack([x0[s[a]] for s in (_p._slice_x, _p._slice_y, _p._slice_psi, _p._slice_phi, _p._slice_v)]) for a in range(4)])
        Rn = 6
        rng = np.random.default_rng(5)
        allrows = np.tile(rows, (Rn, 1)); allW = np.tile(W0, (Rn, 1, 1))
        for r in range(Rn):
            allrows[4 * r + 1, [d2dhip.SC_Y0, d2dhip.SC_Y1]] -= rng.uniform(0.0, 25.0)
            allW[4 * r + 1, 1] = np.linspace(allrows[4 * r + 1, d2dhip.SC_Y0], allrows[4 * r + 1, d2dhip.SC_Y1], W0.shape[2])
        allrows[4 * (Rn - 1):, d2dhip.SC_KCOL] = 0.0
        return allrows, allW, _p.time_step
    finally:
        scen.t1, scen.p0s, scen.p1s, scen.cost = keep


def test_uniform_field_equals_constant_wind(ctx, gold):
    """1. d2d_nlp_solve_groups_wind in uniform_field(c), arbitrary finite start times, against d2d_nlp_solve_groups with c in the rows:
    same statuses and sweep counts, cost within 1e-7 relative, nodes within 1e-5."""
    import d2dhip as D
    rows, W0, h = _joint_scenarios(gold)
    c = (1.0, -0.5)
    rows_c = rows.copy()
    rows_c[:, D.SC_WX], rows_c[:, D.SC_WY] = -c[0], -c[1]            # (the row stores -w)
    Wc = ctx.dev(W0.copy())
    oc = ctx.nlp_solve_groups(ctx.dev(rows_c), Wc, h, 4)
    ctx.sync()
    Wc = Wc.cpu().numpy()
    rows_f = rows.copy()
    rows_f[:, D.SC_WX] = rows_f[:, D.SC_WY] = 123.0                  # ignored in a field
    W, out = _launch(ctx, rows_f, W0, R.uniform_field(c), [3.0, -7.5, 0.0, 1e3, 0.1, 12.0], n_ac=4, h=h)
    cc = oc['cost'].cpu().numpy()
    print('status', out['status'], oc['status'].cpu().numpy(), 'sweeps', out['sweeps'], oc['sweeps'].cpu().numpy())
    print('cost rel', np.abs(out['cost'] - cc) / np.maximum(cc, 1e-3), 'nodes', np.abs(W - Wc).max())
    assert np.array_equal(out['status'], oc['status'].cpu().numpy()) and (out['status'] == 1).all()
    assert np.array_equal(out['sweeps'], oc['sweeps'].cpu().numpy())
    assert (np.abs(out['cost'] - cc) <= 1e-7 * np.maximum(cc, 1e-3)).all()
    assert np.abs(W - Wc).max() <= 1e-5


@pytest.mark.parametrize('name', ['shear', 'vortex', 'gust'])
def test_against_the_cpu_statement(ctx, fields, name):
    """2. The three scenarios of nlp_groups_wind_ref.group_scenarios in one launch (the gust: a different start time per scenario):
    status 1, feas <= 1e-8 reported and recomputed at each scenario's own start time, cost = the reference's cost() of the returned
    nodes to 1e-11, bounds held, cost within 1e-7 relative and nodes within 1e-4 of the statement, sweeps equal.  The partner in
    cost(): aircraft 1's last solve saw aircraft 0's final nodes; aircraft 0's last solve saw aircraft 1 BEFORE aircraft 1's last
    turn, which the kernel leaves in `prev`."""
    F = fields[name]
    ts = G.T_STARTS[name]
    scs, rows, W0 = _batch()
    W, out = _launch(ctx, rows, W0, F, ts)
    for r, sc in enumerate(scs):
        pbs = G.problems_of(sc)
        Ws, infos, sweeps, moved = G.solve_groups(pbs, G.guesses(sc), G.in_field(F, ts[r]))
        print(f'{name} scenario {r}: sweeps {out["sweeps"][r]} / {sweeps}, moved {out["moved"][r]:.2e} / {moved:.2e}')
        assert out['sweeps'][r] == sweeps
        for a in range(N_AC):
            b = N_AC * r + a
            Wi = W[b].T
            pb = pbs[a]
            pb.partner = (out['prev'][r].T.copy() if a == 0 else W[N_AC * r, :2].T.copy()) if a < 2 else None
            fp = R.FieldProblem(pb, F, ts[r])
            feas_np = float(np.abs(R.constraints(fp, Wi)).max())
            print(f'  aircraft {a}: status {out["status"][b]} / {infos[a]["status"]}, cost {out["cost"][b]:.12f} vs {infos[a]["cost"]:.12f} '
                  f'(cost() of the nodes: off by {abs(out["cost"][b] - nlp.cost(pb, Wi)):.1e}), nodes {np.abs(Wi - Ws[a]).max():.2e}, feas {out["feas"][b]:.2e} '
                  f'(numpy {feas_np:.2e}), steps {out["iters"][b]} / {infos[a]["inner"]}')
            assert out['status'][b] == 1 and infos[a]['status'] == 1
            assert out['feas'][b] <= 1e-8 and feas_np <= 1e-8
            assert abs(out['cost'][b] - nlp.cost(pb, Wi)) <= 1e-11 * max(1.0, out['cost'][b])
            assert (Wi >= pb.lo - 1e-15).all() and (Wi <= pb.hi + 1e-15).all()
            assert abs(infos[a]['cost'] - out['cost'][b]) <= 1e-7 * max(infos[a]['cost'], 1e-3)
            assert np.abs(Wi - Ws[a]).max() <= 1e-4
            np.testing.assert_array_equal(Wi[0, :3], pb.p0); np.testing.assert_array_equal(Wi[-1, :3], pb.p1)
        assert np.abs(out['prev'][r] - W[N_AC * r + 1, :2]).max() <= out['moved'][r]          # (what aircraft 1's last turn moved)


@pytest.mark.parametrize('name', ['shear', 'vortex', 'gust'])
def test_joint_kkt_in_the_field(ctx, fields, name):
    """3. Each aircraft of the pair is a KKT point of its sub-problem against the partner's final positions (= joint KKT): the CPU
    solver in the field, started at the kernel's answer with the partner frozen at the kernel's answer, stays there (nodes within
    1e-5) -- every scenario, every field."""
    F = fields[name]
    ts = G.T_STARTS[name]
    scs, rows, W0 = _batch()
    W, out = _launch(ctx, rows, W0, F, ts)
    for r in range(len(scs)):
        pbs = G.problems_of(scs[r])
        for a, o in ((0, 1), (1, 0)):
            pb = pbs[a]
            pb.partner = W[N_AC * r + o, :2].T.copy()
            Wo, info = R.solve(R.FieldProblem(pb, F, ts[r]), W[N_AC * r + a].T.copy())
            d = np.abs(Wo - W[N_AC * r + a].T).max()
            print(f'{name} scenario {r} aircraft {a}: restart moved the nodes by {d:.2e}, cost {info["cost"]:.12f} vs {out["cost"][N_AC * r + a]:.12f}')
            assert info['status'] == 1 and d <= 1e-5


def test_batches_and_repeats_are_bitwise(ctx, fields):
    """4a. Same kernel: R scenarios in one launch equal R single-scenario launches bitwise; two identical launches are bitwise equal."""
    F = fields['gust']
    ts = G.T_STARTS['gust']
    scs, rows, W0 = _batch()
    W, out = _launch(ctx, rows, W0, F, ts)
    W2, out2 = _launch(ctx, rows, W0, F, ts)
    assert np.array_equal(W, W2) and all(np.array_equal(out[k], out2[k]) for k in ('cost', 'feas', 'iters', 'status', 'sweeps', 'moved'))
    for r in range(len(scs)):
        s = slice(N_AC * r, N_AC * r + N_AC)
        W1, o1 = _launch(ctx, rows[s], W0[s], F, ts[r:r + 1])
        assert np.array_equal(W1, W[s]) and np.array_equal(o1['cost'], out['cost'][s]) and np.array_equal(o1['iters'], out['iters'][s])
        assert o1['sweeps'][0] == out['sweeps'][r]


@pytest.mark.parametrize('Nn', [41, 121])
def test_one_aircraft_per_scenario_equals_the_single_aircraft_kernel(ctx, fields, Nn):
    """4b. Other kernel, to rounding: n_ac = 1, all start times equal, against d2d_nlp_solve_wind on field_problems(Nn, 11): same
    status and Newton-step count, cost within 1e-9 relative, nodes within 1e-6."""
    from test_gpu_nlp_wind import _rows
    F = fields['gust']
    pbs, W0s, obs = R.field_problems(Nn, 11)
    rows = np.stack(_rows(pbs, obs))
    W0 = np.stack([w.T for w in W0s])
    Ws = ctx.dev(W0.copy())
    os_ = ctx.nlp_solve_wind(ctx.dev(rows), Ws, pbs[0].h, F, t_start=1.0)
    ctx.sync()
    Ws = Ws.cpu().numpy()
    W, out = _launch(ctx, rows, W0, F, np.full(len(pbs), 1.0), n_ac=1, h=pbs[0].h)
    cs = os_['cost'].cpu().numpy()
    print(f'{Nn} nodes: steps {out["iters"]} / {os_["iters"].cpu().numpy()}, cost rel {np.abs(out["cost"] - cs) / np.maximum(cs, 1e-3)}, '
          f'nodes {np.abs(W - Ws).max():.2e}, bitwise {np.array_equal(W, Ws)}')
    assert np.array_equal(out['status'], os_['status'].cpu().numpy()) and (out['status'] == 1).all()
    assert np.array_equal(out['iters'], os_['iters'].cpu().numpy())
    assert (out['sweeps'] == 0).all()
    assert (np.abs(out['cost'] - cs) <= 1e-9 * np.maximum(cs, 1e-3)).all() and np.abs(W - Ws).max() <= 1e-6


def test_the_start_time_is_per_scenario(ctx, fields):
    """5. The same scenario twice in one launch, from 0 s and from 6 s in the gust: two different plans, each bitwise the plan of a
    single-scenario launch at that time."""
    F = fields['gust']
    scs, rows, W0 = _batch()
    s = slice(N_AC, 2 * N_AC)
    rows2 = np.concatenate([rows[s], rows[s]]); W02 = np.concatenate([W0[s], W0[s]])
    W, out = _launch(ctx, rows2, W02, F, [0.0, 6.0])
    assert (out['status'] == 1).all()
    d = np.abs(W[:N_AC, :2] - W[N_AC:, :2]).max()
    print(f'plans from 0 s and from 6 s differ by {d:.3f} m')
    assert d > 1e-3
    for k, t in enumerate((0.0, 6.0)):
        W1, o1 = _launch(ctx, rows[s], W0[s], F, [t])
        assert np.array_equal(W1, W[N_AC * k:N_AC * k + N_AC]) and np.array_equal(o1['cost'], out['cost'][N_AC * k:N_AC * k + N_AC])


def _track_case(ctx, n, T=80, dt=0.1):
    rng = np.random.default_rng(3)
    t = np.arange(T) * dt
    x0 = rng.uniform(-60, 0, n); y0 = rng.uniform(-80, 40, n); a = rng.uniform(-0.3, 0.3, n)
    x_ref = x0[None] + 12.0 * t[:, None] * np.cos(a)[None]; y_ref = y0[None] + 12.0 * t[:, None] * np.sin(a)[None] + 3.0 * np.sin(0.5 * t)[:, None]
    X0 = np.stack([x_ref[0] + 0.5, y_ref[0] - 0.5, a, np.zeros(n), np.full(n, 12.0)])
    return ctx.dev(np.ascontiguousarray(x_ref)), ctx.dev(np.ascontiguousarray(y_ref)), ctx.dev(np.ascontiguousarray(X0)), dt


def test_tracking_from_per_drone_start_times(ctx, fields):
    """6. d2d_sim_track_run_wind_at: an all-equal start-time tensor against the scalar entry point; two drones with different start
    times against two single-drone scalar launches (every recorded history within 1e-12 absolute); the same launch twice: bitwise."""
    import torch
    F = fields['gust']
    keys = ('X', 'U', 'Xr', 'dX', 'Yd', 'Ydd', 'X_final')
    kw = dict(w=(0.5, -0.3), tau_phi=0.3, tau_v=1.0, wind=F)
    n = 70
    x, y, X0, dt = _track_case(ctx, n)
    oa = ctx.track_run(x, y, X0, dt, t_start=torch.full((n,), 2.5, dtype=torch.float64, device=ctx.device), **kw)
    ob = ctx.track_run(x, y, X0, dt, t_start=2.5, **kw)
    ctx.sync()
    for k in keys:
        d = (oa[k] - ob[k]).abs().max().item()
        print(f'all-equal start times vs the scalar entry point, {k}: {d:.2e}, bitwise {torch.equal(oa[k], ob[k])}')
        assert d <= 1e-12
    x2, y2, X02 = x[:, :2].contiguous(), y[:, :2].contiguous(), X0[:, :2].contiguous()
    t2 = torch.tensor([1.0, 6.5], dtype=torch.float64, device=ctx.device)
    o2 = ctx.track_run(x2, y2, X02, dt, t_start=t2, **kw)
    o2b = ctx.track_run(x2, y2, X02, dt, t_start=t2, **kw)
    ctx.sync()
    assert all(torch.equal(o2[k], o2b[k]) for k in keys)
    for j, tj in enumerate((1.0, 6.5)):
        o1 = ctx.track_run(x2[:, j:j + 1].contiguous(), y2[:, j:j + 1].contiguous(), X02[:, j:j + 1].contiguous(), dt, t_start=tj, **kw)
        ctx.sync()
        for k in keys:
            d = (o2[k][..., j] - o1[k][..., 0]).abs().max().item()
            print(f'drone {j} from {tj} s vs a single-drone scalar launch, {k}: {d:.2e}, bitwise {d == 0.0}')
            assert d <= 1e-12
    assert (o2['X'][..., 0] - ctx.track_run(x2, y2, X02, dt, t_start=6.5, **kw)['X'][..., 0]).abs().max().item() > 1e-6      # the time matters


def test_the_mission_in_a_field(ctx):
    """7. full_sim_phases_batch(windfield=F) for three formations of four aircraft that end phase 1 at different rows, F the field of
    nlp_groups_wind_ref.mission_field: unsteady over the mission's own time span (it grows from 100 s on; phase 1 ends near 134 s), so
    that every time handed from phase to phase is seen by a check: the plan holds its equalities in -F at its OWN formation's start
    time and misses them at another formation's (>= 1e-4: mission_wind's docstring derives 2.5e-4 per row of difference); phases 2 and
    3 are bitwise a direct track_run from per-drone times computed here from the stop rows, and differ from one with the formations'
    times swapped."""
    import torch
    import d2dhip as D
    import full_sim as fs
    import multi_opt_planner as mop
    import d2d.dynamic as ddyn
    F = G.mission_field()
    n_ac, c, X1_f, X2_f, X0B, ref3 = G.mission_inputs()
    time_3 = ref3[0]
    cB = np.stack([c, c, c])
    r, v, t_opt, t_step = 60, 15, 6, 0.05
    dctx = D.default_context()
    ph1 = fs.CircularFormationGVF_batch(cB, r, v, n_ac, X0f=np.stack([X1_f] * 3)[:, :, :3], t_step=t_step, t_end=1000., X0=X0B, record=(), windfield=F)
    dctx.sync()
    stop = ph1['stop_row'].cpu().numpy(); rows_n = len(ph1['time'])
    t_end = G.mission_t_end(stop, rows_n, t_step, t_opt, time_3, 2)          # room for two passes of phase 3
    out = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, ref3=ref3, t_sim_end=t_end, X0=X0B, windfield=F,
                                   record3=('X',))
    dctx.sync()
    assert torch.equal(out['phase1']['X_final'], ph1['X_final'])
    t2h = (np.minimum(stop, rows_n) - 1) * t_step
    print('stop rows', stop, 'start times of the plans', t2h)
    assert len(set(stop.tolist())) == 3 and (stop < rows_n).all()
    assert 100.0 + 2.0 < t2h.min() and t2h.max() + t_opt + 2 * time_3[-1] < 210.0           # the whole mission inside the field's unsteady span
    t2 = out['plan']['t_start'].cpu().numpy()
    np.testing.assert_array_equal(t2, t2h)
    st = out['plan']['status'].cpu().numpy()
    print('status', st, 'sweeps', out['plan']['sweeps'].cpu().numpy(), 'feas', out['plan']['feas'].cpu().numpy())
    assert (st == 1).all()
    Xs = out['plan']['Xs'].cpu().numpy()                         # (12, 5, K)
    Xf1 = ph1['X_final'].cpu().numpy().T                         # (12, 5)
    rows = out['plan']['scen'].cpu().numpy()
    Fm = -F
    for b in range(3 * n_ac):
        pb = nlp.problem_from_row(rows[b], Xs.shape[2], 0.1)
        res = [float(np.abs(R.constraints(R.FieldProblem(pb, Fm, t2h[f]), Xs[b].T)).max()) for f in range(3)]
        print(f'drone {b}: collocation residual at the start time of formation 0, 1, 2: {res[0]:.2e} {res[1]:.2e} {res[2]:.2e}')
        for f in range(3):
            assert (res[f] <= 1e-8) if f == b // n_ac else (res[f] >= 1e-4), (b, f, res)
        np.testing.assert_array_equal(Xs[b, :3, 0], Xf1[b, :3])
        np.testing.assert_array_equal(Xs[b, :3, -1], np.tile(X2_f[:, :3], (3, 1))[b])
        assert np.abs(Xs[b, 3]).max() <= rows[b, D.SC_PHIMAX] and Xs[b, 4].min() >= rows[b, D.SC_VMIN] and Xs[b, 4].max() <= rows[b, D.SC_VMAX]
    # phases 2 and 3 against direct launches from per-drone times computed HERE, on the host, from the stop rows
    W = out['plan']['Xs']
    ac = ddyn.Aircraft()
    kw = dict(w=(0., 0.), tau_phi=ac.tau_phi, tau_v=ac.tau_v, wind=F)
    t2d = np.repeat(t2h, n_ac)
    x2, y2 = W[:, 0, :].t().contiguous(), W[:, 1, :].t().contiguous()
    ph2 = dctx.track_run(x2, y2, ph1['X_final'], 0.1, record=('X', 'U'), t_start=dctx.dev(t2d), **kw)
    ph2_swapped = dctx.track_run(x2, y2, ph1['X_final'], 0.1, record=('X',), t_start=dctx.dev(np.repeat(np.roll(t2h, 1), n_ac)), **kw)
    dctx.sync()
    assert torch.equal(ph2['X'], out['phase2']['X']) and torch.equal(ph2['U'], out['phase2']['U']) and torch.equal(ph2['X_final'], out['phase2']['X_final'])
    d2 = (ph2_swapped['X'] - out['phase2']['X']).abs().max().item()
    print(f'phase 2 flown from the other formations\' start times differs by {d2:.2e} m')
    assert d2 > 1e-9
    assert len(out['phase3']) == 2
    x3 = dctx.dev(np.tile(np.ascontiguousarray(ref3[1]), (1, 3))); y3 = dctx.dev(np.tile(np.ascontiguousarray(ref3[2]), (1, 3)))
    X_last = out['phase2']['X_final']
    dur2 = 6.0
    for k in range(2):
        tk = t2d + (dur2 + k * float(time_3[-1]))
        ph3 = dctx.track_run(x3, y3, X_last, 0.1, record=('X',), t_start=dctx.dev(tk), **kw)
        ph3_swapped = dctx.track_run(x3, y3, X_last, 0.1, record=('X',), t_start=dctx.dev(np.repeat(np.roll(t2h, 1), n_ac) + (dur2 + k * float(time_3[-1]))), **kw)
        ph3_late = dctx.track_run(x3, y3, X_last, 0.1, record=('X',), t_start=dctx.dev(tk + float(time_3[-1])), **kw)
        dctx.sync()
        assert torch.equal(ph3['X'], out['phase3'][k]['X']) and torch.equal(ph3['X_final'], out['phase3'][k]['X_final'])
        d3 = (ph3_swapped['X'] - out['phase3'][k]['X']).abs().max().item(); d3l = (ph3_late['X'] - out['phase3'][k]['X']).abs().max().item()
        print(f'phase 3 pass {k}: from the other formations\' times differs by {d3:.2e} m, from one pass later by {d3l:.2e} m')
        assert d3 > 1e-9 and d3l > 1e-9
        X_last = out['phase3'][k]['X_final']
    err = (out['phase2']['X_final'][:2] - W[:, :2, -1].t()).abs().max().item()
    print(f'end of phase 2 vs the end of the plan: {err:.3f} m')
    # windfield=None is today's path
    a = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, X0=X0B)
    b = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, X0=X0B, windfield=None)
    dctx.sync()
    assert torch.equal(a['plan']['Xs'], b['plan']['Xs']) and torch.equal(a['phase2']['X'], b['phase2']['X']) and 'status' not in b['plan']


def test_validation(ctx, fields):
    """8. NULL field, bad field, NULL t_start: D2D_EINVAL naming the entry point, nothing launched; a NaN start time: that scenario
    D2D_ST_NONFINITE (cost = feas = NaN), the others solved."""
    import d2dhip
    scs, rows, W0 = _batch()
    dsc = ctx.dev(rows[:N_AC].copy()); W = ctx.dev(W0[:N_AC].copy())
    t = ctx.dev(np.zeros(1))
    good = fields['shear'].device_field(ctx)
    for bad in (dict(nx=3), dict(nt=2), dict(hx=0.0), dict(hy=-1.0), dict(cp=None)):
        f = d2dhip.WindFieldC(good.nt, good.ny, good.nx, 0, good.t0, good.ht, good.x0, good.hx, good.y0, good.hy, good.cp)
        for k, v in bad.items():
            setattr(f, k, v)
        with pytest.raises(d2dhip.D2DError, match='d2d_nlp_solve_groups_wind'):
            ctx.nlp_solve_groups_wind(dsc, W, H, N_AC, f, t)
    with pytest.raises(d2dhip.D2DError, match='d2d_nlp_solve_groups_wind'):
        ctx.nlp_solve_groups_wind(dsc, W, H, N_AC, None, t)
    with pytest.raises(d2dhip.D2DError, match='d2d_nlp_solve_groups_wind.*t_start'):
        ctx.nlp_solve_groups_wind(dsc, W, H, N_AC, fields['shear'], None)
    ctx.sync()
    np.testing.assert_array_equal(W.cpu().numpy(), W0[:N_AC])         # nothing ran
    x, y, X0, dt = _track_case(ctx, 3)
    with pytest.raises(d2dhip.D2DError, match='d2d_sim_track_run_wind_at'):
        p = ctx.track_params(3, x.shape[0], dt)
        d2dhip._check(ctx.lib.d2d_sim_track_run_wind_at(ctx.h, d2dhip.C.byref(p), x.data_ptr(), y.data_ptr(), X0.data_ptr(), None, None, None,
                                                        None, None, None, None, d2dhip.C.byref(good), None, None))
    with pytest.raises(AssertionError, match='need a wind field'):
        ctx.track_run(x, y, X0, dt, t_start=ctx.dev(np.zeros(3)))
    Wn, out = _launch(ctx, rows, W0, fields['shear'], [0.0, np.nan, 0.0])
    s = slice(N_AC, 2 * N_AC)
    assert (out['status'][s] == d2dhip.ST_NONFINITE).all() and np.isnan(out['cost'][s]).all() and np.isnan(out['feas'][s]).all()
    assert (out['iters'][s] == 0).all() and np.array_equal(Wn[s], W0[s])
    keep = np.r_[0:N_AC, 2 * N_AC:3 * N_AC]
    assert (out['status'][keep] == 1).all() and np.isfinite(out['cost'][keep]).all()
