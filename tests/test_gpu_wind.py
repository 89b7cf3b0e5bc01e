"""GPU: wind fields that vary in space and time (include/d2d.h d2d_wind_field, ABI 111) through the C ABI, against the CPU
references of tests/wind_ref.py -- (a) the kernels' algorithm in numpy, (b) the reference's continuous model under DOP853 -- in
three fields: a linear shear, a Gaussian vortex (steady) and a gust that varies in time.  Measured values beside the asserts."""
import numpy as np
import pytest

import wind_ref as R
from oracle import sim as S

pytestmark = pytest.mark.gpu

GUST_T = np.arange(0.0, 30.01, 0.5)


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return {'shear': R.spline_of(R.shear), 'vortex': R.spline_of(R.vortex), 'gust': R.spline_of(R.gust, t=GUST_T)}


def _planes(a):
    return np.ascontiguousarray(np.asarray(a, float).T)


def _states(n, seed, box=100.0):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-box, box, n), rng.uniform(-box, box, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.7, 0.7, n),
                  rng.uniform(8, 16, n)], 1)
    dphi = np.where(rng.random(n) < 0.5, rng.uniform(-S.GL_FAST_DPHI, S.GL_FAST_DPHI, n), rng.uniform(-0.5, 0.5, n))
    U = np.stack([X[:, 3] - dphi, rng.uniform(9, 16, n)], 1)
    return X, U


def test_wind_sample_matches_numpy(ctx, fields):
    rng = np.random.default_rng(1)
    n = 10000
    t = rng.uniform(-2.0, 34.0, n)
    xy = np.stack([rng.uniform(-180, 180, n), rng.uniform(-230, 180, n)])          # inside and (clamped) outside the box
    for name, f in fields.items():
        w = ctx.wind_sample(f, ctx.dev(t), ctx.dev(xy)).cpu().numpy()
        wx, wy = f.sample_many(t, xy[0], xy[1])
        assert np.abs(w[0] - wx).max() <= 1e-13 and np.abs(w[1] - wy).max() <= 1e-13, name      # measured <= 4e-15


def test_wind_field_validation(ctx, fields):
    import d2dhip
    f = fields['gust'].device_field(ctx)
    t, xy = ctx.zeros(4), ctx.zeros(2, 4)
    for k, v in (('nx', 3), ('ny', 2), ('nt', 2), ('nt', 0), ('hx', 0.0), ('hy', -1.0), ('ht', 0.0), ('cp', None)):
        g = d2dhip.WindFieldC.from_buffer_copy(f)
        setattr(g, k, v)
        with pytest.raises(d2dhip.D2DError, match='wind field'):
            ctx.wind_sample(g, t, xy)
        with pytest.raises(d2dhip.D2DError, match='wind field'):
            ctx.step_wind(ctx.zeros(5, 4), ctx.zeros(2, 4), 0.0, g)


@pytest.mark.parametrize('tau_phi', [0.01, 0.9667])
def test_step_wind_vs_references(ctx, fields, tau_phi):
    """d2d_step_wind on 4096 random states (half of them on the one-panel branch) against (a) and, on a subset, (b)."""
    import torch
    X, U = _states(4096, 3)
    for name, f in fields.items():
        t0 = 4.2
        it = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        o = ctx.step_wind(ctx.dev(_planes(X)), ctx.dev(_planes(U)), t0, f, tau_phi, 1.0, 0.05, iter_max=it).cpu().numpy().T
        Xa, ita = R.disc_dyn_glrk_wind(X, U, f, t0, 0.05, tau_phi, 1.0, return_iters=True)
        d = o - Xa; d[:, 2] = S.norm_mpi_pi(d[:, 2])
        assert np.abs(d).max() <= 1e-11, (name, np.abs(d).max())                # measured <= 5e-14
        assert 1 <= int(it.item()) <= 6 and int(it.item()) >= ita.max(), (name, int(it.item()), ita.max())   # measured 4
        sub = np.arange(0, 4096, 128)
        Xb = np.array([R.disc_dyn_ivp_wind(X[i], U[i], f, t0, 0.05, tau_phi, 1.0) for i in sub])
        d = o[sub] - Xb; d[:, 2] = S.norm_mpi_pi(d[:, 2])
        assert np.abs(d).max() <= 2e-9, (name, np.abs(d).max())                 # measured 8e-10 (tau_phi 0.01), 3e-14 (0.9667)


def test_uniform_spline_field_equals_constant_step(ctx):
    from d2d.wind import SplineWindField
    X, U = _states(4096, 9)
    w = (0.7, -0.4)
    f = SplineWindField(np.stack([np.full((6, 7), w[0]), np.full((6, 7), w[1])])[None], -200.0, 60.0, -200.0, 80.0)
    dX, dU = ctx.dev(_planes(X)), ctx.dev(_planes(U))
    for tau in (0.01, 0.9667):
        a = ctx.step_wind(dX, dU, 1.5, f, tau, 1.0, 0.05).cpu().numpy()
        b = ctx.step(dX, dU, w, tau, 1.0, 0.05).cpu().numpy()
        d = np.abs(a - b)
        # The weights of a B-spline sum to one only up to rounding: the winds differ by ~1e-16 and a position by the odd ulp per
        # panel.  1e-14 is below one ulp of |x| >= 64 (1.4e-14): the bound is in ulps of the result.
        assert (d <= 4 * np.spacing(np.abs(b))).all() and d.max() <= 6e-14, d.max()      # measured max 1.4e-14 (1 ulp at |x| = 74)
        assert np.abs(a[:, np.abs(b[:2]).max(0) < 32] - b[:, np.abs(b[:2]).max(0) < 32]).max() <= 1e-14


def _gvf_setup(n_ac, seed=5):
    if n_ac == 4:        # src/09_CircularFormation_diffcentre.py (tests/test_gpu_sim.py)
        c = np.array([[0, -20], [25, -40], [25, -80], [0, -100.0]])
        X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (4, 1))
        return c, X0, 60.0, 15.0
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20, 20, (n_ac, 2))
    X0 = np.zeros((n_ac, 5))
    X0[:, 0] = rng.uniform(10, 40, n_ac); X0[:, 1] = rng.uniform(10, 40, n_ac); X0[:, 2] = rng.uniform(-3, 3, n_ac); X0[:, 4] = 12.0
    return c, X0, 50.0, 13.0


@pytest.mark.parametrize('n_ac,n_form', [(4, 3), (33, 2), (1, 5), (2, 5)])
@pytest.mark.parametrize('field', ['vortex', 'gust'])
def test_gvf_closed_loop_in_a_field(ctx, fields, n_ac, n_form, field):
    """400 steps of the formation loop flown through the field (the GVF law sees no wind), identical formations in partial blocks
    (4: 12 of 64 lanes; 33: 66 of 256; 1 and 2: 5 and 10 of 64 -- formations that only the wind path sends to the general
    LDS-exchange kernel), against (a) in the same closed loop."""
    import full_sim as fs
    f = fields[field]
    T, dt, t0 = 401, 0.05, 1.0
    c, X0, r, v = _gvf_setup(n_ac)
    out = fs.CircularFormationGVF_batch(np.tile(c[None], (n_form, 1, 1)), r, v, n_ac, t_start=t0, t_step=dt, t_end=t0 + (T - 0.5) * dt,
                                        X0=np.tile(X0[None], (n_form, 1, 1)), windfield=f)
    assert len(out['time']) == T
    ctx.sync()
    import d2dhip
    d2dhip.default_context().sync()
    Xh = out['X'].cpu().numpy().transpose(0, 2, 1).reshape(T, n_form, n_ac, 5)
    U = out['U'].cpu().numpy().transpose(0, 2, 1).reshape(T, n_form, n_ac, 2)
    Xo, Uo, it_o = R.formation_gvf_run_wind(c, r, v, X0, T, dt, f, t_start=t0)
    for k in range(n_form):
        d = Xh[:, k] - Xo; d[..., 2] = S.norm_mpi_pi(d[..., 2])
        assert np.abs(d).max() <= 1e-8, (k, np.abs(d).max())                      # measured <= 3e-11
        assert np.abs(U[:T - 1, k] - Uo[:T - 1]).max() <= 1e-9                    # measured <= 6e-12
    it = int(out['iter_max'].item())
    assert 1 <= it <= 6, it                                                       # measured 4 (a: 4)
    # and the field is felt: the same loop in the wind at the formation's first position differs by metres
    w0 = f.sample(t0, X0[0, :2])
    Xc, *_ = S.formation_gvf_run(c, r, v, X0, T, dt, W=w0)
    assert np.abs(Xc[..., :2] - Xo[..., :2]).max() > 1.0


@pytest.mark.parametrize('n_ac,n_form', [(4, 3), (33, 2)])
def test_gvf_wind_loop_is_repeatable(ctx, fields, n_ac, n_form):
    """The same wind run twice -- wavefronts that mix the one-panel and graded meshes, the gust's unsteady sum -- gives bitwise
    equal histories (an earlier out-of-line field evaluation did not)."""
    f = fields['gust']
    T, dt = 201, 0.05
    c, X0, r, v = _gvf_setup(n_ac)
    N = n_ac * n_form
    dX0, dC, dR = ctx.dev(_planes(np.tile(X0, (n_form, 1)))), ctx.dev(_planes(np.tile(c, (n_form, 1)))), ctx.dev(np.full(N, r))
    runs = [ctx.gvf_run(dX0, dC, dR, n_ac, T, dt, v, wind=f, t_start=2.0) for _ in range(2)]
    ctx.sync()
    for k in ('X', 'U', 'Rr', 'X_final'):
        assert np.array_equal(runs[0][k].cpu().numpy(), runs[1][k].cpu().numpy()), k


def test_tracking_loop_in_a_field(ctx, fields, gold):
    """implement_controller_batch(windfield=): the plant flies the shear, the controller keeps DiffController(w)'s constant w."""
    import full_sim as fs
    import d2dhip
    g = gold('tracking_trace_carestandin')
    time = g['time']; w = (0.5, -0.3)
    out = fs.implement_controller_batch(time, g['x_ref'], g['y_ref'], w, g['X'][0], windfield=fields['shear'])
    d2dhip.default_context().sync()
    X = out['X'].cpu().numpy().transpose(0, 2, 1); U = out['U'].cpu().numpy().transpose(0, 2, 1)
    Xr = out['Xr'].cpu().numpy().transpose(0, 2, 1)
    Xo, Uo, Xro = R.track_run_wind(time, g['x_ref'], g['y_ref'], g['X'][0], w, fields['shear'])
    T = len(time)
    d = X - Xo; d[..., 2] = S.norm_mpi_pi(d[..., 2])
    assert np.abs(d).max() < 1e-7, np.abs(d).max()                               # tests/test_gpu_sim.py tolerances
    np.testing.assert_allclose(U[:T - 1], Uo[:T - 1], atol=1e-6)
    np.testing.assert_allclose(Xr[:T - 1], Xro[:T - 1], atol=1e-7)
    assert 1 <= int(out['iter_max'].item()) <= 6


def _dfff_case():
    import d2d.trajectory as ddt
    J = [np.array([[0., 0.], [12., 0.], [0., 0.], [0., 0.]]).T,
         np.array([[40., 10.], [12., 1.], [0.2, -0.1], [0., 0.]]).T,
         np.array([[80., -5.], [12., -1.], [0., 0.3], [0., 0.]]).T]
    traj = ddt.CompositeTraj([ddt.MinSnapPoly(J[j], J[j + 1], 3.5) for j in range(2)])
    time = np.arange(0, 7.0 - 1e-9, 0.05)
    perts = np.zeros((len(time), 5)); perts[30] = [0.5, -0.4, 0.03, 0.0, 0.2]
    X0 = np.array([0.5, -1.0, 0.05, 0.0, 11.5])
    return traj, time, perts, X0


def test_dfff_loop_in_a_field(ctx, fields):
    """run_simulation with a SplineWindField: the plant flies the vortex, the controller samples it at the reference point."""
    import full_sim as fs
    import d2d.dynamic as ddyn
    import d2d.guidance as ddg
    traj, time, perts, X0 = _dfff_case()
    f = fields['vortex']
    ac = ddyn.Aircraft()
    X, U, Yref = fs.run_simulation(time, ac, f, ddg.DFFFController(traj, ac, f), X0, perts)
    Xo, Uo, _ = R.dfff_run_wind(time, Yref, X0, f, perts)
    d = X - Xo; d[:, 2] = S.norm_mpi_pi(d[:, 2])
    assert np.abs(d).max() < 1e-7, np.abs(d).max()
    np.testing.assert_allclose(U, Uo, atol=1e-6)


def test_run_simulation_flies_a_time_varying_gust():
    """The mirror: full_sim.run_simulation in a gust that varies in time equals a host loop of DFFFController.get and (a) steps --
    what Aircraft.disc_dyn does with a SplineWindField -- and differs by more than a metre from the same run in the wind frozen at
    time[0] (what the loop flew before fields existed)."""
    import full_sim as fs
    import d2d.dynamic as ddyn
    import d2d.guidance as ddg
    from d2d.wind import SplineWindField
    traj, time, perts, X0 = _dfff_case()
    gust = R.spline_of(lambda t, x, y: R.gust(t, x, y, t_peak=3.5, amp=5.0), t=GUST_T)
    assert isinstance(gust, SplineWindField)
    ac = ddyn.Aircraft()
    X, U, Yref = fs.run_simulation(time, ac, gust, ddg.DFFFController(traj, ac, gust), X0, perts)
    ctl = ddg.DFFFController(traj, ac, gust)
    Xh = np.zeros_like(X); Uh = np.zeros_like(U); Xh[0] = X0
    for i in range(1, len(time)):
        Uh[i - 1] = ctl.get(Xh[i - 1].copy(), time[i - 1])
        Xh[i] = R.disc_dyn_glrk_wind(Xh[i - 1], Uh[i - 1], gust, time[i - 1], time[i] - time[i - 1]) + perts[i]
    Uh[-1] = ctl.get(Xh[-1].copy(), time[-1])
    d = X - Xh; d[:, 2] = S.norm_mpi_pi(d[:, 2])
    assert np.abs(d).max() <= 1e-8, np.abs(d).max()                              # measured <= 1e-11
    np.testing.assert_allclose(U, Uh, atol=1e-8)
    # Aircraft.disc_dyn itself takes the field (d2d_step_wind) along the same trajectory
    for i in (1, 40, 90):
        Xs = ac.disc_dyn(Xh[i - 1], Uh[i - 1], gust, time[i - 1], time[i] - time[i - 1])
        d = Xs - R.disc_dyn_glrk_wind(Xh[i - 1], Uh[i - 1], gust, time[i - 1], time[i] - time[i - 1])
        assert np.abs(d).max() <= 1e-11
    frozen = ddg.WindField(list(gust.sample(time[0], Yref[0, 0])))
    Xf, _, _ = fs.run_simulation(time, ac, frozen, ddg.DFFFController(traj, ac, frozen), X0, perts)
    assert np.abs(Xf[:, :2] - X[:, :2]).max() > 1.0, np.abs(Xf[:, :2] - X[:, :2]).max()      # measured 1.2 m
