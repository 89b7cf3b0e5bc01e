"""GPU: stochastic gusts inside the time loops (include/d2d.h d2d_gust, ABI 118) against the CPU statement tests/gust_ref.py:
the process alone (d2d_gust_sample), the formation loop in constant wind and in a field (d2d_sim_gvf_run_gust), formations that
freeze at different rows of one block, the tracking loop (d2d_sim_track_run_gust), the sigma = 0 twins, the mission chain and the
refusals.  Tolerances: those of tests/test_gpu_wind.py's closed loops; everything the device alone decides is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gust_ref as G
import wind_ref as R
from oracle import sim as S

pytestmark = pytest.mark.gpu

SEED, DT, CORR = 20241008, 0.05, 0.36
W_CONST = (0.5, -0.3)


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return {'shear': R.spline_of(R.shear), 'vortex': R.spline_of(R.vortex), 'gust': R.spline_of(R.gust, t=np.arange(0.0, 30.01, 0.5))}


def _model(sigma=1.5, corr=CORR):
    from d2d.wind import GustModel
    return GustModel(sigma, tau=2.0, seed=SEED, form_corr=corr)


def _planes(a):
    return np.ascontiguousarray(np.asarray(a, float).T)


def _gvf_setup(n_ac, seed=5):
    """the formations of tests/test_gpu_wind.py"""
    if n_ac == 4:
        c = np.array([[0, -20], [25, -40], [25, -80], [0, -100.0]])
        X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (4, 1))
        return c, X0, 60.0, 15.0
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20, 20, (n_ac, 2))
    X0 = np.zeros((n_ac, 5))
    X0[:, 0] = rng.uniform(10, 40, n_ac); X0[:, 1] = rng.uniform(10, 40, n_ac); X0[:, 2] = rng.uniform(-3, 3, n_ac); X0[:, 4] = 12.0
    return c, X0, 50.0, 13.0


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. the process alone -----------------------------------------------------------------------------------------------------
def test_gust_sample_matches_the_cpu_statement_and_continues_bit_for_bit(ctx):
    m = _model()
    N, n_ac, T, phase, base = 129, 3, 65, 2, 3 * 2 ** 31                 # the high stream word is used
    out = ctx.gust_sample(m, N, T, DT, n_ac=n_ac, phase=phase, stream_base=base)
    ctx.sync()
    g = out['g'].cpu().numpy(); gs = out['gust_state'].cpu().numpy()
    go, gso = G.sample(m.numbers(DT), N, T, n_ac, phase, stream_base=base)
    print('g vs the CPU statement', np.abs(g - go).max(), 'state', np.abs(gs - gso[-1]).max(), 'max |g|', np.abs(g).max())
    assert np.abs(g - go).max() <= 1e-12 and np.abs(gs - gso[-1]).max() <= 1e-12
    assert np.abs(g).max() > 1.0                                         # (and they are gusts, not zeros)
    # the shared planes are the same numbers on the aircraft of a formation
    assert _bits(gs[2:].reshape(2, N // n_ac, n_ac), np.repeat(gs[2:].reshape(2, N // n_ac, n_ac)[:, :, :1], n_ac, 2))
    # rows 0 .. 32, then a second call from state_out: rows 32 .. 64 of the one call
    a = ctx.gust_sample(m, N, 33, DT, n_ac=n_ac, phase=phase, stream_base=base)
    b = ctx.gust_sample(m, N, 33, DT, n_ac=n_ac, phase=phase, stream_base=base, state=a['gust_state'], step_base=32)
    ctx.sync()
    assert _bits(a['g'].cpu().numpy(), g[:33]) and _bits(b['g'].cpu().numpy(), g[32:])
    assert _bits(b['gust_state'].cpu().numpy(), gs)
    # streams 30 .. 59 on their own
    s = ctx.gust_sample(m, 30, T, DT, n_ac=n_ac, phase=phase, stream_base=base + 30)
    ctx.sync()
    assert _bits(s['g'].cpu().numpy(), g[:, :, 30:60]) and _bits(s['gust_state'].cpu().numpy(), gs[:, 30:60])
    # without a shared part the shared call is not made: the planes stay zero and g is the own process
    o = ctx.gust_sample(_model(corr=0.0), N, 9, DT, n_ac=n_ac, phase=phase, stream_base=base)
    ctx.sync()
    os_ = o['gust_state'].cpu().numpy()
    assert not os_[2:].any() and _bits(o['g'].cpu().numpy()[-1], os_[:2])
    assert np.abs(o['g'].cpu().numpy() - G.sample(_model(corr=0.0).numbers(DT), N, 9, n_ac, phase, stream_base=base)[0]).max() <= 1e-12


# ---- 2. the formation loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_ac,n_form', [(3, 5), (33, 2), (4, 3)])
@pytest.mark.parametrize('wind', ['constant', 'vortex'])
def test_formation_loop_through_gusts(ctx, fields, n_ac, n_form, wind):
    """401 rows; every formation the same circles and start, its own gusts.  (4, 3): formations the constant-wind twin sends to the
    quad kernel and only the gust sends to the general one."""
    m = _model()
    T, t0, phase = 401, 1.0, 0
    c, X0, r, v = _gvf_setup(n_ac)
    N = n_ac * n_form
    f = None if wind == 'constant' else fields[wind]
    dX0, dC, dR = ctx.dev(_planes(np.tile(X0, (n_form, 1)))), ctx.dev(_planes(np.tile(c, (n_form, 1)))), ctx.dev(np.full(N, r))
    kw = dict(W=W_CONST) if f is None else dict(wind=f, t_start=t0)
    out = ctx.gvf_run(dX0, dC, dR, n_ac, T, DT, v, record=('X', 'U', 'g'), gust=m, gust_phase=phase, **kw)
    calm = ctx.gvf_run(dX0, dC, dR, n_ac, T, DT, v, record=('X',), gust=_model(sigma=0.0), gust_phase=phase, **kw)
    series = ctx.gust_sample(m, N, T, DT, n_ac=n_ac, phase=phase)
    ctx.sync()
    Xh = out['X'].cpu().numpy().transpose(0, 2, 1).reshape(T, n_form, n_ac, 5)
    Uh = out['U'].cpu().numpy().transpose(0, 2, 1).reshape(T, n_form, n_ac, 2)
    g = out['g'].cpu().numpy()
    assert _bits(g, series['g'].cpu().numpy()) and _bits(out['gust_state'].cpu().numpy(), series['gust_state'].cpu().numpy())
    assert (out['stop_row'].cpu().numpy() == T).all()
    Xo, Uo, Go, _, gso = G.formation_gvf_run_gust(c, r, v, X0, T, DT, m.numbers(DT), phase, n_form=n_form, W=W_CONST, field=f, t_start=t0)
    d = Xh - Xo; d[..., 2] = S.norm_mpi_pi(d[..., 2])
    print(n_ac, wind, 'X', np.abs(d).max(), 'U', np.abs(Uh[:T - 1] - Uo[:T - 1]).max(), 'g', np.abs(g - Go).max())
    assert np.abs(d).max() <= 1e-8, np.abs(d).max()
    assert np.abs(Uh[:T - 1] - Uo[:T - 1]).max() <= 1e-9
    assert np.abs(g - Go).max() <= 1e-12 and np.abs(out['gust_state'].cpu().numpy() - gso).max() <= 1e-12
    assert np.abs(Xo[:, 0] - Xo[:, 1]).max() > 1e-3                      # (every formation flies its own gusts)
    # the gust is flown: 1000 times the parity bar
    dc = (out['X'][:, :2] - calm['X'][:, :2]).abs().max().item()
    print('against the sigma = 0 run', dc)
    assert dc > 1e-5
    if f is not None:
        assert 1 <= int(out['iter_max'].item()) <= 6


# ---- 3. formations that freeze at different rows of one block -------------------------------------------------------------------
def test_a_frozen_formation_keeps_its_gust(ctx):
    """Three formations of three aircraft in one 256-thread block, rule 1 with X0f[f] = the CPU statement's state at rows 120, 200
    and 333 and stop_tol 1e-3: each freezes at its own row while its lanes keep looping with the block."""
    m = _model()
    n_ac, n_form, T, phase = 3, 3, 401, 0
    rows = (120, 200, 333)
    tol = (1e-3, 1e-3, 1e-3)
    c, X0, r, v = _gvf_setup(n_ac)
    N = n_ac * n_form
    Xfree, *_ = G.formation_gvf_run_gust(c, r, v, X0, T, DT, m.numbers(DT), phase, n_form=n_form, W=W_CONST)
    X0f = np.stack([Xfree[rows[k], k, :, :3] for k in range(n_form)])
    Xo, _, _, stop_o, gso = G.formation_gvf_run_gust(c, r, v, X0, T, DT, m.numbers(DT), phase, n_form=n_form, W=W_CONST, X0f=X0f, stop_tol=tol)
    assert stop_o.tolist() == [q + 1 for q in rows], stop_o              # the CPU statement stops there: rows [:stop] are kept
    ref = [(Xo[stop_o[k] - 1, k], gso[:, k * n_ac:(k + 1) * n_ac]) for k in range(n_form)]
    dX0, dC, dR = ctx.dev(_planes(np.tile(X0, (n_form, 1)))), ctx.dev(_planes(np.tile(c, (n_form, 1)))), ctx.dev(np.full(N, r))
    out = ctx.gvf_run(dX0, dC, dR, n_ac, T, DT, v, W=W_CONST, X0f=ctx.dev(_planes(X0f.reshape(N, 3))), stop_tol=tol, record=('X', 'g'),
                      gust=m, gust_phase=phase)
    ctx.sync()
    stop = out['stop_row'].cpu().numpy()
    print('stop rows', stop)
    assert stop.tolist() == [q + 1 for q in rows]
    gs = out['gust_state'].cpu().numpy(); Xf = out['X_final'].cpu().numpy().T.reshape(n_form, n_ac, 5)
    for k in range(n_form):
        s = ctx.gust_sample(m, n_ac, int(stop[k]), DT, n_ac=n_ac, phase=phase, stream_base=k * n_ac)       # the state after step stop - 1
        ctx.sync()
        assert _bits(gs[:, k * n_ac:(k + 1) * n_ac], s['gust_state'].cpu().numpy()), k
        assert _bits(out['g'].cpu().numpy()[:stop[k], :, k * n_ac:(k + 1) * n_ac], s['g'].cpu().numpy()), k
        d = Xf[k] - ref[k][0]; d[:, 2] = S.norm_mpi_pi(d[:, 2])
        print(k, 'X_final', np.abs(d).max(), 'state vs the CPU statement', np.abs(gs[:, k * n_ac:(k + 1) * n_ac] - ref[k][1]).max())
        assert np.abs(d).max() <= 1e-8
        assert np.abs(gs[:, k * n_ac:(k + 1) * n_ac] - ref[k][1]).max() <= 1e-12


# ---- 4. the tracking loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['constant', 'shear', 't_start'])
def test_tracking_loop_through_gusts(ctx, fields, gold, case):
    """The tracking_trace_carestandin reference in constant w, in the shear and -- a start time per drone -- in the time-varying field."""
    import torch
    g0 = gold('tracking_trace_carestandin')
    time = g0['time']; w = W_CONST
    x_ref, y_ref, X0 = g0['x_ref'], g0['y_ref'], g0['X'][0]
    T, n = x_ref.shape
    m = _model(sigma=0.8)
    n_ac = 2 if n % 2 == 0 else 1
    f = {'constant': None, 'shear': fields['shear'], 't_start': fields['gust']}[case]
    ts = np.linspace(2.0, 6.5, n) if case == 't_start' else None
    kw = {}
    if f is not None:
        kw = dict(wind=f, t_start=float(time[0]) if ts is None else ctx.dev(ts))
    out = ctx.track_run(ctx.dev(np.ascontiguousarray(x_ref)), ctx.dev(np.ascontiguousarray(y_ref)), ctx.dev(_planes(X0)), float(time[1] - time[0]),
                        record=('X', 'U', 'Xr', 'g'), w=w, gust=m, gust_phase=1, gust_n_ac=n_ac, **kw)
    series = ctx.gust_sample(m, n, T, float(time[1] - time[0]), n_ac=n_ac, phase=1)
    ctx.sync()
    assert torch.equal(out['g'], series['g']) and torch.equal(out['gust_state'], series['gust_state'])
    X = out['X'].cpu().numpy().transpose(0, 2, 1); U = out['U'].cpu().numpy().transpose(0, 2, 1); Xr = out['Xr'].cpu().numpy().transpose(0, 2, 1)
    Xo, Uo, Xro, Go, _ = G.track_run_gust(time, x_ref, y_ref, X0, w, m.numbers(float(time[1] - time[0])), 1, n_ac=n_ac, field=f, t_start=ts)
    d = X - Xo; d[..., 2] = S.norm_mpi_pi(d[..., 2])
    print(case, 'X', np.abs(d).max(), 'U', np.abs(U[:T - 1] - Uo[:T - 1]).max(), 'Xr', np.abs(Xr[:T - 1] - Xro[:T - 1]).max())
    assert np.abs(d).max() < 1e-7, np.abs(d).max()
    np.testing.assert_allclose(U[:T - 1], Uo[:T - 1], atol=1e-6)
    np.testing.assert_allclose(Xr[:T - 1], Xro[:T - 1], atol=1e-7)
    assert np.abs(out['g'].cpu().numpy() - Go).max() <= 1e-12
    # and the gust is flown
    import d2dhip
    twin = ctx.track_run(ctx.dev(np.ascontiguousarray(x_ref)), ctx.dev(np.ascontiguousarray(y_ref)), ctx.dev(_planes(X0)), float(time[1] - time[0]),
                         record=('X',), w=w, **kw)
    ctx.sync()
    assert (twin['X'][:, :2] - out['X'][:, :2]).abs().max().item() > 1e-4
    assert isinstance(m.lower(0.1, 1), d2dhip.GustC)


# ---- 5. sigma = 0: the twins ----------------------------------------------------------------------------------------------------
def test_a_calm_gust_is_the_twin_bit_for_bit(ctx, fields, gold):
    import torch
    calm = _model(sigma=0.0)
    n_ac, n_form, T = 3, 5, 201
    c, X0, r, v = _gvf_setup(n_ac)
    N = n_ac * n_form
    X0s = np.tile(X0, (n_form, 1)); X0s[:, :2] += np.arange(N)[:, None] * 0.37          # every formation its own flight
    dX0, dC, dR = ctx.dev(_planes(X0s)), ctx.dev(_planes(np.tile(c, (n_form, 1)))), ctx.dev(np.full(N, r))
    zero = ctx.zeros(4, N)
    for kw in (dict(W=W_CONST), dict(wind=fields['vortex'], t_start=1.0), dict(wind=fields['gust'], t_start=2.0)):
        a = ctx.gvf_run(dX0, dC, dR, n_ac, T, DT, v, gust=calm, gust_state=zero, **kw)
        b = ctx.gvf_run(dX0, dC, dR, n_ac, T, DT, v, **kw)
        ctx.sync()
        for k in ('X', 'U', 'Rr', 'eth', 'X_final', 'stop_row'):
            assert torch.equal(a[k], b[k]), (sorted(kw), k, (a[k] - b[k]).abs().max().item())
        assert not a['gust_state'].any()
    g0 = gold('tracking_trace_carestandin')
    time = g0['time']; dt = float(time[1] - time[0])
    x, y, X0t = ctx.dev(np.ascontiguousarray(g0['x_ref'])), ctx.dev(np.ascontiguousarray(g0['y_ref'])), ctx.dev(_planes(g0['X'][0]))
    n = x.shape[1]
    zero = ctx.zeros(4, n)
    ts = ctx.dev(np.linspace(2.0, 6.5, n))
    for kw in (dict(), dict(wind=fields['shear'], t_start=0.0), dict(wind=fields['gust'], t_start=2.5), dict(wind=fields['gust'], t_start=ts)):
        a = ctx.track_run(x, y, X0t, dt, w=W_CONST, gust=calm, gust_state=zero, **kw)
        b = ctx.track_run(x, y, X0t, dt, w=W_CONST, **kw)
        ctx.sync()
        for k in ('X', 'U', 'Xr', 'dX', 'Yd', 'Ydd', 'X_final'):
            assert torch.equal(a[k], b[k]), (sorted(kw), k, (a[k] - b[k]).abs().max().item())


# ---- 6. the mission chain -------------------------------------------------------------------------------------------------------
def test_the_mission_chain_hands_the_gust_on(ctx):
    """full_sim_phases_batch(gust=, audit=True) on two formations of tests/test_gpu_mission_wind.py's mission: the state goes from
    phase 1 to phase 2 to each repetition of phase 3 under the phase words 0, 1, 2 + k; sigma = 0 is the chain without gust=."""
    import torch
    import d2dhip as D
    import full_sim as fs
    import multi_opt_planner as mop
    import nlp_groups_wind_ref as GW
    n_ac, c, X1_f, X2_f, X0B, ref3 = GW.mission_inputs()
    time_3 = ref3[0]
    cB, X0B = np.stack([c, c]), X0B[:2]
    r, v, t_opt, t_step = 60, 15, 6, 0.05
    dctx = D.default_context()
    m = _model(sigma=0.3)

    def one_pass(**kw):
        """t_sim_end that leaves room for exactly one repetition of phase 3 after this phase 1"""
        ph1 = fs.CircularFormationGVF_batch(cB, r, v, n_ac, X0f=np.stack([X1_f] * 2)[:, :, :3], t_step=t_step, t_end=1000., X0=X0B, record=(), **kw)
        dctx.sync()
        return ph1, GW.mission_t_end(ph1['stop_row'].cpu().numpy(), len(ph1['time']), t_step, t_opt, time_3, 1)

    _, t_end = one_pass()
    base = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, ref3=ref3, t_sim_end=t_end, X0=X0B, record3=('X',))
    dctx.sync()
    assert len(base['phase3']) == 1
    calm = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, ref3=ref3, t_sim_end=t_end, X0=X0B, record3=('X',),
                                    gust=_model(sigma=0.0))
    dctx.sync()
    assert torch.equal(calm['phase1']['X_final'], base['phase1']['X_final']) and torch.equal(calm['phase1']['stop_row'], base['phase1']['stop_row'])
    assert torch.equal(calm['plan']['Xs'], base['plan']['Xs']) and torch.equal(calm['plan']['cost'], base['plan']['cost'])
    for k in ('X', 'U', 'X_final'):
        assert torch.equal(calm['phase2'][k], base['phase2'][k]), k
    assert len(calm['phase3']) == 1 and all(torch.equal(a['X'], b['X']) and torch.equal(a['X_final'], b['X_final'])
                                            for a, b in zip(calm['phase3'], base['phase3']))
    ph1g, t_end = one_pass(gust=m)
    out = fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, ref3=ref3, t_sim_end=t_end, X0=X0B, record2=('X', 'U', 'g'),
                                   record3=('X', 'g'), gust=m, audit=True)
    dctx.sync()
    N = 2 * n_ac
    gs = out['phase1']['gust_state']
    assert tuple(gs.shape) == (4, N) and gs.abs().max().item() > 0
    chain = [out['phase2']] + out['phase3']
    assert len(out['phase3']) == 1
    for k, ph in enumerate(chain):
        # row 0 of the loop's g is the combination of the state it was handed; a one-row sample from that state is that combination
        one = dctx.gust_sample(m, N, 1, 0.1, n_ac=n_ac, phase=1 + k, state=gs)
        dctx.sync()
        assert torch.equal(ph['g'][0], one['g'][0]), k
        T = ph['g'].shape[0]
        ser = dctx.gust_sample(m, N, T, 0.1, n_ac=n_ac, phase=1 + k, state=gs)
        dctx.sync()
        assert torch.equal(ph['g'], ser['g']) and torch.equal(ph['gust_state'], ser['gust_state']), k
        gs = ph['gust_state']
    # phase 1's state is the series of phase word 0 at each formation's own last executed step
    stop = out['phase1']['stop_row'].cpu().numpy(); rows_n = len(out['phase1']['time'])
    for f in range(2):
        s = dctx.gust_sample(m, n_ac, int(min(stop[f], rows_n)), t_step, n_ac=n_ac, phase=0, stream_base=f * n_ac)
        dctx.sync()
        assert torch.equal(s['gust_state'], out['phase1']['gust_state'][:, f * n_ac:(f + 1) * n_ac]), f
    a = out['audit']
    assert set(a) == {'plan', 'phase2', 'phase3'} and len(a['phase3']) == len(out['phase3'])
    for d in [a['plan'], a['phase2']] + a['phase3']:
        assert (d['status'] == 0).all() and torch.isfinite(d['sep_dist']).all()
    assert torch.equal(out['phase1']['X_final'], ph1g['X_final']) and torch.equal(out['phase1']['gust_state'], ph1g['gust_state'])
    assert (out['phase1']['X_final'][:2] - base['phase1']['X_final'][:2]).abs().max().item() > 1e-5           # the gust is flown


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import d2dhip
    m = _model()
    N, n_ac, T = 12, 3, 9
    good = m.lower(DT, n_ac, 0, 0)
    bad = [('sigma', -1.0), ('sigma', np.nan), ('sigma', np.inf), ('s', -1e-3), ('s', np.nan), ('a', 1.0), ('a', -1e-9), ('a', np.nan),
           ('w_own', np.nan), ('w_form', np.inf), ('w_own', -good.w_own), ('w_form', -good.w_form), ('w_own', good.w_own + 1e-9), ('n_ac', 0),
           ('n_ac', 5), ('stream_base', 4), ('stream_base', -3), ('phase', -1), ('step_base', -1), ('step_base', 2 ** 32)]
    c, X0, r, v = _gvf_setup(n_ac)
    n_form = N // n_ac
    dX0, dC, dR = ctx.dev(_planes(np.tile(X0, (n_form, 1)))), ctx.dev(_planes(np.tile(c, (n_form, 1)))), ctx.dev(np.full(N, r))
    x, y = ctx.zeros(T, N), ctx.zeros(T, N)
    mark = 123.456

    def outs(keys, shapes):
        o = {k: ctx.zeros(*s) + mark for k, s in zip(keys, shapes)}
        o['stop_row'] = o['conv_row'] = None
        return o

    def untouched(o):
        ctx.sync()
        return all((t == mark).all().item() for t in o.values() if t is not None)

    for k, val in bad:
        g = d2dhip.GustC.from_buffer_copy(good)
        setattr(g, k, val)
        buf = outs(('g', 'gust_state'), ((T, 2, N), (4, N)))
        g.state_out, g.g_hist = buf['gust_state'].data_ptr(), buf['g'].data_ptr()
        rc = ctx.lib.d2d_gust_sample(ctx.h, N, T, C.byref(g))
        assert rc == -1 and untouched(buf), ('d2d_gust_sample', k, val, rc)
        o = outs(('X', 'U', 'Rr', 'eth', 'X_final', 'gust_state', 'g'), ((T, 5, N), (T, 2, N), (T, N), (T, n_form * 2), (5, N), (4, N), (T, 2, N)))
        with pytest.raises(d2dhip.D2DError, match='d2d_sim_gvf_run_gust'):
            ctx.gvf_run(dX0, dC, dR, n_ac, T, DT, v, out=o, record=('X', 'U', 'Rr', 'eth', 'g'), gust=g)
        assert untouched(o), ('d2d_sim_gvf_run_gust', k, val)
        o = outs(('X', 'U', 'Xr', 'dX', 'Yd', 'Ydd', 'X_final', 'gust_state', 'g'),
                 ((T, 5, N), (T, 2, N), (T, 5, N), (T, 5, N), (T, 2, N), (T, 2, N), (5, N), (4, N), (T, 2, N)))
        with pytest.raises(d2dhip.D2DError, match='d2d_sim_track_run_gust'):
            ctx.track_run(x, y, dX0, DT, out=o, gust=g)
        assert untouched(o), ('d2d_sim_track_run_gust', k, val)
    # gust NULL
    assert ctx.lib.d2d_gust_sample(ctx.h, N, T, None) == -1
    p = ctx.track_params(N, T, DT)
    o = outs(('X_final',), ((5, N),))
    assert ctx.lib.d2d_sim_track_run_gust(ctx.h, C.byref(p), x.data_ptr(), y.data_ptr(), dX0.data_ptr(), None, None, None, None, None, None,
                                          o['X_final'].data_ptr(), None, None, None, None) == -1 and untouched(o)
    gp = d2dhip.GvfParams(n_form, n_ac, T, 1, DT, 0.01, 1.0, 4e-4, 25.0, 20.0, v, 0.0, 0.0, 0, 0, (C.c_double * 3)(3.0, 3.0, 0.01))
    B = np.ascontiguousarray(S.construct_b_matrix(n_ac)); z = np.zeros(n_ac - 1)
    assert ctx.lib.d2d_sim_gvf_run_gust(ctx.h, C.byref(gp), dX0.data_ptr(), dC.data_ptr(), dR.data_ptr(), B.ctypes.data_as(C.c_void_p),
                                        z.ctypes.data_as(C.c_void_p), None, None, None, None, None, o['X_final'].data_ptr(), None, None, None, 0.0,
                                        None, None) == -1 and untouched(o)
    assert 'null gust' in ctx.lib.d2d_last_error().decode()
    # nothing to write
    g = d2dhip.GustC.from_buffer_copy(good)
    assert ctx.lib.d2d_gust_sample(ctx.h, N, T, C.byref(g)) == -1 and 'both NULL' in ctx.lib.d2d_last_error().decode()
    # N no multiple of n_ac
    buf = outs(('gust_state',), ((4, N + 1),))
    g.state_out = buf['gust_state'].data_ptr()
    assert ctx.lib.d2d_gust_sample(ctx.h, N + 1, T, C.byref(g)) == -1 and untouched(buf)
    # and the good struct is accepted
    g.state_out = buf['gust_state'].data_ptr()
    assert ctx.lib.d2d_gust_sample(ctx.h, N, T, C.byref(g)) == 0
    ctx.sync()
