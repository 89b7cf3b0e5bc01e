"""GPU parity: the collocation backend in a wind field that varies in space and time (d2d_nlp_solve_wind, csrc/nlp_kernels.hip
nlp_solve_wind_kernel) against
  * d2d_nlp_solve and oracle/nlp.py in a spatially uniform field (a constant wind),
  * the CPU statement of the solver in a field (tests/nlp_wind_ref.py) in a shear, a vortex and an unsteady gust,
  * the KKT conditions in the field,
and the planner on top of it.  The tolerances are those tests/test_gpu_nlp.py holds the constant-wind kernel to."""
import numpy as np
import pytest

import nlp_wind_ref as R
from oracle import nlp, costs as C
from test_gpu_nlp import _row

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return R.fields()


def _solve_wind(ctx, pbs, W0s, rows, field, t_start=0.0, **kw):
    """W0s: (N, 5) per problem -> device [B][5][N]; returns the solution as (N, 5, B), the outputs and mult as (N, 3, B)."""
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s], 0)))
    out = ctx.nlp_solve_wind(ctx.dev(np.stack(rows)), W, pbs[0].h, field, t_start=t_start, want_mult=True, **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k != 'work'}
    res['mult'] = np.ascontiguousarray(res['mult'].transpose(2, 1, 0))
    return np.ascontiguousarray(W.cpu().numpy().transpose(2, 1, 0)), res


def _rows(pbs, obs):
    rows = [_row(pb, ob, 1.0 if ob else 0.0, 0) for pb, ob in zip(pbs, obs)]
    for r in rows:                                   # the row's wind columns are not read in a field
        import d2dhip as D
        r[D.SC_WX] = r[D.SC_WY] = np.nan
    return rows


def _check_against_statement(pb, field, t_start, Wi, out, i, W0, node_tol=1e-4):
    fp = R.FieldProblem(pb, field, t_start)
    Wo, info = R.solve(fp, W0)
    feas_np = float(np.abs(R.constraints(fp, Wi)).max())
    lam = 2 * info['rho'] * out['mult'][1:, :, i]
    kkt, _ = R.kkt_residual(fp, Wi, lam, info['zL'], info['zU'])
    print(f'  problem {i}: status {out["status"][i]} / {info["status"]}, cost {out["cost"][i]:.12f} vs {info["cost"]:.12f}, nodes {np.abs(Wi - Wo).max():.2e}, '
          f'feas {out["feas"][i]:.2e} (numpy {feas_np:.2e}), steps {out["iters"][i]} / {info["inner"]}, kkt {kkt:.2e}')
    assert info['status'] == 1 and out['status'][i] == 1, (i, out['status'][i], info['status'])
    assert out['feas'][i] <= 1e-8 and feas_np <= 1e-8
    assert abs(out['cost'][i] - nlp.cost(pb, Wi)) <= 1e-11 * max(1.0, out['cost'][i])
    assert (Wi >= pb.lo - 1e-15).all() and (Wi <= pb.hi + 1e-15).all()
    assert abs(info['cost'] - out['cost'][i]) <= 1e-7 * max(info['cost'], 1e-3), (i, info['cost'], out['cost'][i])
    assert np.abs(Wi - Wo).max() <= node_tol, (i, np.abs(Wi - Wo).max())
    assert abs(int(out['iters'][i]) - info['inner']) <= 10, (i, out['iters'][i], info['inner'])
    assert kkt <= 1e-5, (i, kkt)
    return Wo, info


def test_uniform_field_equals_constant_wind(ctx):
    """The batch of test_batch_with_obstacles_wind_and_boxes_vs_oracle (7 problems, 41 nodes, both obstacle kinds, a binding y box),
    every problem in the uniform field c = (1, -0.5): d2d_nlp_solve_wind against d2d_nlp_solve with wind = c in the row (same status,
    cost within 1e-7 relative, nodes within 1e-5) and against oracle.nlp.solve at that test's tolerances."""
    import d2dhip as D
    N, h = 41, 0.1
    c = (1.0, -0.5)
    pbs, rows, W0s = [], [], []
    rng = np.random.default_rng(4)
    for i in range(7):
        p0 = (0., 0., rng.uniform(-0.5, 0.5), 0., 12.); p1 = (48. + rng.uniform(-4, 4), rng.uniform(-6, 6), rng.uniform(-0.4, 0.4), 0., 12.)
        ob = [(24. + rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 7))] if i % 2 else []
        kind = 0 if i == 3 else 1
        pb = nlp.Problem(N, h, p0, p1, vsp=12., kv=5., kphi=1., obj_scale=0.1 if i < 4 else 1.0, wind=c,
                         phi_max=np.deg2rad(35.), v_min=9., v_max=15., y_box=(-6.5, 9.) if i == 5 else None, obstacles=ob,
                         kobs=1.0 if ob else 0.0, obs_kind=kind)
        pbs.append(pb); rows.append(_row(pb, ob, 1.0 if ob else 0.0, 1 if kind == 0 and ob else 0))
        W0s.append(nlp.from_free(C.single_guess('tri', p0, p1, 12., (N - 1) * h, N), N))
    Wc = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s], 0)))
    oc = ctx.nlp_solve(ctx.dev(np.stack(rows)), Wc, h)
    ctx.sync()
    Wc = Wc.cpu().numpy().transpose(2, 1, 0)
    rows_f = [r.copy() for r in rows]
    for r in rows_f:
        r[D.SC_WX] = r[D.SC_WY] = 123.0              # ignored in a field
    W, out = _solve_wind(ctx, pbs, W0s, rows_f, R.uniform_field(c), t_start=3.0)
    for i, pb in enumerate(pbs):
        Wi = W[:, :, i]
        cc = float(oc['cost'][i].item())
        print(f'  problem {i}: cost {out["cost"][i]:.12f} vs constant kernel {cc:.12f}, nodes {np.abs(Wi - Wc[:, :, i]).max():.2e}')
        assert out['status'][i] == 1 and int(oc['status'][i].item()) == 1
        assert abs(out['cost'][i] - cc) <= 1e-7 * max(cc, 1e-3) and np.abs(Wi - Wc[:, :, i]).max() <= 1e-5
        assert out['feas'][i] <= 1e-8 and np.abs(nlp.constraints(pb, Wi)).max() <= 1e-8
        assert abs(out['cost'][i] - nlp.cost(pb, Wi)) <= 1e-11 * max(1.0, out['cost'][i])
        assert (Wi >= pb.lo - 1e-15).all() and (Wi <= pb.hi + 1e-15).all()
        Wo, info = nlp.solve(pb, W0s[i])
        assert info['status'] == 1
        assert abs(info['cost'] - out['cost'][i]) <= 1e-7 * max(info['cost'], 1e-3), (i, info['cost'], out['cost'][i])
        assert np.abs(Wi - Wo).max() <= 1e-4, (i, np.abs(Wi - Wo).max())
        kkt, feas = nlp.kkt_residual(pb, Wi, 2 * info['rho'] * out['mult'][1:, :, i], info['zL'], info['zU'])
        assert kkt <= 1e-5 and feas <= 1e-8, (i, kkt)


@pytest.mark.parametrize('name', ['shear', 'vortex', 'gust'])
@pytest.mark.parametrize('N', [41, 121])
def test_shear_vortex_gust_vs_cpu_statement(ctx, fields, name, N):
    """Ragged batches (tests/nlp_wind_ref.py field_problems: 4 / 3 problems per launch, an obstacle on every second row) in the three
    fields of tests/wind_ref.py; the gust is unsteady and starts at t_start = 1 s.  Every problem converges in the CPU statement
    (chosen so on the CPU) and must on the device: status 1, feas <= 1e-8 reported and recomputed with sample_many, cost = the
    reference's cost() of the returned nodes to 1e-11, bounds held, cost within 1e-7 relative and nodes within 1e-4 of the
    statement, Newton steps within +-10, KKT residual in the field with the returned multipliers <= 1e-5."""
    F = fields[name]
    t_start = 1.0 if name == 'gust' else 0.0
    pbs, W0s, obs = R.field_problems(N, 11)
    W, out = _solve_wind(ctx, pbs, W0s, _rows(pbs, obs), F, t_start=t_start)
    print(f'{name}, {N} nodes')
    for i, pb in enumerate(pbs):
        _check_against_statement(pb, F, t_start, W[:, :, i], out, i, W0s[i])
        np.testing.assert_allclose(W[0, :3, i], pb.p0, atol=0); np.testing.assert_allclose(W[-1, :3, i], pb.p1, atol=0)


def test_the_field_is_not_frozen(ctx, fields):
    """The first 121-node shear problem solved in the field and solved by d2d_nlp_solve with the field frozen at its value at the
    start pose: the plans differ.  The CPU statement against oracle/nlp.py in the frozen wind shows 4.94 m (largest distance between
    nodes of the same index); asserted: more than 0.4 m."""
    import d2dhip as D
    F = fields['shear']
    pbs, W0s, obs = R.field_problems(121, 11)
    pb, W0 = pbs[0], W0s[0]
    W, out = _solve_wind(ctx, [pb], [W0], _rows([pb], [obs[0]]), F)
    wf = F.sample(0.0, (pb.p0[0], pb.p0[1]))
    row = _row(pb, obs[0], 0.0, 0)
    row[D.SC_WX], row[D.SC_WY] = -wf[0], -wf[1]
    Wz = ctx.dev(np.ascontiguousarray(W0.T[None]))
    oz = ctx.nlp_solve(ctx.dev(row[None]), Wz, pb.h)
    ctx.sync()
    Wz = Wz.cpu().numpy()[0].T
    d = float(np.hypot(W[:, 0, 0] - Wz[:, 0], W[:, 1, 0] - Wz[:, 1]).max())
    print(f'field vs frozen at the start pose: {d:.3f} m')
    assert out['status'][0] == 1 and int(oz['status'][0].item()) == 1
    assert d > 0.4, d                                   # (measured on the CPU: 4.94 m)


@pytest.mark.parametrize('N', [3, 63, 64, 65, 129, 200])
def test_ragged_node_counts_in_a_field_vs_cpu_statement(ctx, fields, N):
    """The twin of test_ragged_node_counts_vs_oracle in the steady shear: node counts around the chunk size of the node-parallel
    phases (64: the hand-over of the field's value between lanes and between chunks) and beyond the LDS records (> 121)."""
    h = 0.1
    # (the side-step of the twin at 10 m/s over the ground: the shear's ~2 m/s act against the leg, and its 0.5 m/s across it carry
    # the end point along -- with three nodes there is no room to fly anything else)
    p0 = (0., 0., 0., 0., 12.); p1 = (10. * h * (N - 1) * 0.995, (0.01 if N <= 5 else 0.15) * (N - 1) - 0.5 * h * (N - 1), 0., 0., 12.)
    pb = nlp.Problem(N, h, p0, p1, vsp=12., kv=1., kphi=5., obj_scale=float(N), phi_max=np.deg2rad(30.), v_min=9., v_max=15.)
    W0 = np.stack([np.linspace(p0[0], p1[0], N), np.linspace(p0[1], p1[1], N), np.zeros(N), np.zeros(N), np.full(N, 12.)], 1)
    W, out = _solve_wind(ctx, [pb], [W0], _rows([pb], [[]]), fields['shear'])
    _check_against_statement(pb, fields['shear'], 0.0, W[:, :, 0], out, 0, W0, node_tol=1e-5)
    np.testing.assert_allclose(W[0, :3, 0], p0[:3], atol=0); np.testing.assert_allclose(W[-1, :3, 0], p1[:3], atol=0)


def test_serial_recursion_and_order_in_a_field(ctx, fields):
    """serial = 1 (the twisted block recursion) gives the cyclic reduction's result to rounding, and a hand-out order only schedules
    (bitwise the same W with two slots and the reversed order), both in the unsteady field."""
    import torch
    F = fields['gust']
    pbs, W0s, obs = R.field_problems(41, 11)
    rows = _rows(pbs, obs)
    W, out = _solve_wind(ctx, pbs, W0s, rows, F, t_start=1.0)
    Ws, outs = _solve_wind(ctx, pbs, W0s, rows, F, t_start=1.0, serial=1)
    assert (out['status'] == 1).all() and (outs['status'] == 1).all()
    print(f'serial vs cyclic reduction: nodes {np.abs(W - Ws).max():.2e}, cost {np.abs(out["cost"] - outs["cost"]).max():.2e}')
    assert np.abs(W - Ws).max() <= 1e-6 and (np.abs(out['cost'] - outs['cost']) <= 1e-9 * np.maximum(out['cost'], 1e-3)).all()
    order = torch.arange(len(pbs) - 1, -1, -1, dtype=torch.int32, device=ctx.device)
    Wr, outr = _solve_wind(ctx, pbs, W0s, rows, F, t_start=1.0, order=order, slots=2)
    assert np.array_equal(W, Wr) and np.array_equal(out['cost'], outr['cost']) and np.array_equal(out['iters'], outr['iters'])


def test_repeatable(ctx, fields):
    """The same batch solved twice: bitwise-equal W, in a steady and in the unsteady field (the guard DESIGN 5.9 added)."""
    for name, N in (('vortex', 121), ('gust', 41)):
        pbs, W0s, obs = R.field_problems(N, 11)
        rows = _rows(pbs, obs)
        W1, o1 = _solve_wind(ctx, pbs, W0s, rows, fields[name], t_start=0.5)
        W2, o2 = _solve_wind(ctx, pbs, W0s, rows, fields[name], t_start=0.5)
        assert np.array_equal(W1, W2) and np.array_equal(o1['cost'], o2['cost']) and np.array_equal(o1['iters'], o2['iters'])


def test_planner_end_to_end_in_a_field(ctx, fields, tmp_path):
    """Planner(exp_14-like, wind = -F).run(): the collocation problem in the field answers ('nlp', status 1), the plan is feasible in
    -F, save_solution writes the field along the plan and load_solution reads the plan back."""
    import d2d.optyplan_scenarios as d2oscen
    import single_opt_planner as sop
    Fm = -fields['shear']

    class windy(d2oscen.exp_14):
        wind = Fm
    p = sop.Planner(windy)
    p.run()
    assert p.info['backend_used'] == 'nlp' and p.info['status'] == 1, p.info
    W = np.stack([p.sol_x, p.sol_y, p.sol_psi, p.sol_phi, p.sol_v], 1)
    pb = nlp.Problem(121, 0.1, windy.p0, windy.p1, vsp=12., kv=1., kphi=0., phi_max=np.deg2rad(40.), v_min=9., v_max=15.,
                     x_box=(-150, 150), y_box=(-150, 150))
    fp = R.FieldProblem(pb, Fm, 0.0)
    assert np.abs(R.constraints(fp, W)).max() <= 1e-8 and p.info['feas'] <= 1e-8
    assert abs(p.info['obj_val'] - nlp.cost(pb, W)) <= 1e-12
    assert np.abs(p.sol_phi).max() <= np.deg2rad(40.) and p.sol_v.min() >= 9. and p.sol_v.max() <= 15.
    # the field matters: the plan in still air has another cost
    Wo, info = R.solve(fp, nlp.from_free(p.get_initial_guess('tri'), 121))
    assert info['status'] == 1 and abs(info['cost'] - p.info['obj_val']) <= 1e-7 * info['cost']
    fn = str(tmp_path / 'plan.npz')
    p.save_solution(fn)
    d = np.load(fn)
    wx, wy = Fm.sample_many(p.sol_time, p.sol_x, p.sol_y)
    np.testing.assert_array_equal(d['wind'], np.stack([wx, wy], 1))
    q = sop.Planner(windy)
    q.load_solution(fn)
    np.testing.assert_array_equal(q.sol_x, p.sol_x); np.testing.assert_array_equal(q.sol_v, p.sol_v)


def test_validation(ctx, fields):
    """A bad field and f == NULL give D2D_EINVAL (a D2DError naming the entry point), as for the other *_wind entry points."""
    import d2dhip
    pbs, W0s, obs = R.field_problems(41, 11)
    rows = ctx.dev(np.stack(_rows(pbs[:1], obs[:1])))
    W = ctx.dev(np.ascontiguousarray(W0s[0].T[None]))
    good = fields['shear'].device_field(ctx)
    for bad in (dict(nx=3), dict(nt=2), dict(hx=0.0), dict(hy=-1.0), dict(cp=None)):
        f = d2dhip.WindFieldC(good.nt, good.ny, good.nx, 0, good.t0, good.ht, good.x0, good.hx, good.y0, good.hy, good.cp)
        for k, v in bad.items():
            setattr(f, k, v)
        with pytest.raises(d2dhip.D2DError, match='d2d_nlp_solve_wind'):
            ctx.nlp_solve_wind(rows, W, 0.1, f)
    with pytest.raises(d2dhip.D2DError, match='null wind field'):
        ctx.nlp_solve_wind(rows, W, 0.1, None)
    work = ctx.empty(ctx.lib.d2d_nlp_workspace_doubles(41))
    rc = ctx.lib.d2d_nlp_solve_wind(ctx.h, 1, 41, 0.1, rows.data_ptr(), None, W.data_ptr(), work.data_ptr(), None, work.data_ptr(),
                                    work.data_ptr(), None, None, None, 0.0)
    assert rc == -1                                       # D2D_EINVAL
    ctx.sync()
    np.testing.assert_array_equal(W.cpu().numpy()[0].T, W0s[0])       # nothing ran
