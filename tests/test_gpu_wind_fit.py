"""GPU: d2d_wind_fit against its CPU statement tests/wind_fit_ref.py -- H and b bit for bit against the fixed-point replay, within the
documented quantisation against plain fp64, the solve against the reference system, order independence, refusals, recovery."""
import numpy as np
import pytest

import wind_fit_ref as WF

pytestmark = pytest.mark.gpu

N_FORM, N_AC, N_ROWS, DT = 3, 4, 130, 0.05
ROWS = np.array([130, 65, 1], dtype=np.int32)          # two chunk boundaries and a remainder; half; a formation without a sample
T_START = np.array([0.0, 3.0, 7.5])
W_MAX, LAM, MU, CG_TOL = 30.0, (1e-2, 2e-2, 5e-3), 1e-4, 1e-10
GRIDS = {                                              # boxes around the histories of _history(): x in [-120, 120], y in [-100, 100]
    'steady-4x4': WF.Grid(1, 4, 4, 0.0, 1.0, -120.0, 240.0, -100.0, 200.0),          # a single cell
    'steady-5x6': WF.Grid(1, 5, 6, 0.0, 1.0, -120.0, 80.0, -100.0, 100.0),           # cells change inside a chunk
    'unsteady-4x5x6': WF.Grid(4, 5, 6, -1.0, 16.0, -120.0, 80.0, -100.0, 100.0),
}


def _history(seed=3):
    """12 drones on arcs through a wind that varies in space, 130 rows: not a simulation, any history is one.  Drone 0 has a NaN
    row, drone 1 leaves the box, drone 2 jumps (a measurement above w_max)."""
    rng = np.random.default_rng(seed)
    N = N_FORM * N_AC
    t = np.arange(N_ROWS) * DT
    X = np.zeros((N_ROWS, 5, N))
    for d in range(N):
        v, om, psi0, xs = rng.uniform(9.0, 14.0), rng.uniform(-0.35, 0.35), rng.uniform(-np.pi, np.pi), rng.uniform(-25.0, 25.0)
        if d == 1:
            om, psi0, xs = 0.0, 0.0, 110.0                           # straight out of the box through x = 120
        psi = psi0 + om * t
        x = xs + np.cumsum(np.r_[0.0, (v * np.cos(psi[:-1]) + 2.0) * DT])
        y = rng.uniform(-20.0, 20.0) + np.cumsum(np.r_[0.0, (v * np.sin(psi[:-1]) - 1.0 + 0.02 * x[:-1]) * DT])
        X[:, 0, d], X[:, 1, d], X[:, 2, d], X[:, 3, d], X[:, 4, d] = x, y, psi + 40.0 * np.pi * (d % 3), 0.1 * om, v
    X[17, 3, 0] = np.nan
    X[70:, 1, 2] += 4.0
    return X


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def hist():
    return _history()


def _grid_c(g, cp=None):
    import d2dhip
    return d2dhip.WindFieldC(g.nt, g.ny, g.nx, 0, g.t0, g.ht, g.x0, g.hx, g.y0, g.hy, cp)


def _fit(ctx, X, g, rows=ROWS, t_start=T_START, prior=None, outputs=('support', 'stats', 'H', 'b'), **kw):
    import torch
    dX = X if hasattr(X, 'data_ptr') else ctx.dev(X)
    dr = None if rows is None else ctx.dev(np.asarray(rows, dtype=np.int32), dtype=torch.int32)
    dt0 = None if t_start is None else ctx.dev(np.asarray(t_start, dtype=np.float64))
    dp = None if prior is None else ctx.dev(prior)
    args = dict(w_max=W_MAX, lam=LAM, mu=MU, cg_tol=CG_TOL, cg_max=4000)
    args.update(kw)
    out = ctx.wind_fit(dX, N_AC, DT, _grid_c(g), rows=dr, t_start=dt0, prior=dp, outputs=outputs, **args)
    ctx.sync()
    return {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in out.items()}


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope='module')
def refs(hist):
    """The CPU statement of every grid, computed once: measurements, A, the replayed sums, the reference system."""
    out = {}
    for name, g in GRIDS.items():
        ms = WF.measure(hist, N_AC, DT, g, ROWS, T_START, W_MAX)
        A, m = WF.design(ms, g)
        out[name] = dict(ms=ms, A=A, m=m, replay=WF.replay(ms, g, W_MAX))
    return out


@pytest.mark.parametrize('name', list(GRIDS))
def test_sums_are_the_fixed_point_replay_bit_for_bit(ctx, hist, refs, name):
    """H_out, b_out and the counts are those of wind_fit_ref.replay exactly; support is the diagonal.  The history holds every
    rejection: a NaN row (two samples), a drone that leaves the box, a jump above w_max."""
    g, ref = GRIDS[name], refs[name]
    got = _fit(ctx, hist, g)
    Hs, bs, _, _ = ref['replay']
    counts = ref['ms']['counts']
    assert counts[0] > 500 and counts[1] == 2 and counts[2] > 0 and counts[3] == 1
    assert list(got['stats'][:4]) == [float(c) for c in counts]
    assert _bits(got['H'], Hs)
    assert _bits(got['b'], bs)
    assert _bits(got['support'], Hs[:, Hs.shape[1] // 2])
    if name == 'steady-5x6':
        cells = {tuple(s) for s in ref['ms']['seg'][:, ref['ms']['why'] == 0].T}
        assert len(cells) > 1                                        # the cell does change inside a chunk


@pytest.mark.parametrize('name', list(GRIDS))
def test_sums_against_plain_fp64_and_the_solve_against_the_reference_system(ctx, hist, refs, name):
    """Against A^T A and A^T m in plain fp64: each entry sums at most S products, each rounded once to a multiple of 2^-32 (error
    <= 2^-33; for b times W = 32, w_max rounded up to a power of two), and the fp64 reference's own summation of S terms of at most
    1 (W) errs by at most S^2 2^-53 (W).  The solve: the residual of the REFERENCE system at the kernel's control points is at most
    cg_tol |rhs| plus what the perturbation of H and b moves, |dH|_F |c| + |db|, times 4."""
    g, ref = GRIDS[name], refs[name]
    got = _fit(ctx, hist, g)
    A, m = ref['A'], ref['m']
    S = ref['ms']['counts'][0]
    W = WF.w_pow2(W_MAX)
    assert W == 32.0
    qH = S * 2.0 ** -33 + S * S * 2.0 ** -53
    qb = qH * W
    H = (A.T @ A).tocsr()
    b = np.stack([A.T @ m[0], A.T @ m[1]])
    dH, db = np.abs(got['H'] - WF.stencil_of(H, g)).max(), np.abs(got['b'] - b).max()
    print(f'{name}: S = {S}, |dH| = {dH:.3e} (bound {qH:.3e}), |db| = {db:.3e} (bound {qb:.3e})')
    assert dH <= qH and db <= qb
    M, rhs = WF.system(H, b, g, LAM, MU)
    ncp = g.nt * g.ny * g.nx
    c = got['cp'].transpose(1, 0, 2, 3).reshape(2, ncp)
    assert got['stats'][6] < 4000 and got['stats'][7] <= CG_TOL
    for k in range(2):
        res = np.linalg.norm(M @ c[k] - rhs[k])
        bound = 4.0 * (CG_TOL * np.linalg.norm(rhs[k]) + qH * np.sqrt(got['H'].size) * np.linalg.norm(c[k]) + qb * np.sqrt(ncp))
        print(f'  component {k}: |M c - rhs| = {res:.3e} (bound {bound:.3e}), {int(got["stats"][6])} CG iterations')
        assert res <= bound
    # the residual sums of squares: the fitted field at the used samples (fp64 sums of S terms)
    rss = [float(np.sum((A @ c[k] - m[k]) ** 2)) for k in range(2)]
    assert np.allclose(got['stats'][4:6], rss, rtol=1e-9, atol=1e-12 * S)


def test_outputs_do_not_depend_on_the_order_of_the_work(ctx, hist):
    """Bit-identical cp, support, H, b and counts: on a repeated call, for other launch geometries (1, 3, 7 wavefronts and the
    library's choice), and under a permutation of the formations with rows and t_start permuted alike."""
    for name, g in GRIDS.items():
        base = _fit(ctx, hist, g)
        perm = [2, 0, 1]
        Xp = np.ascontiguousarray(hist.reshape(N_ROWS, 5, N_FORM, N_AC)[:, :, perm].reshape(N_ROWS, 5, -1))
        others = [_fit(ctx, hist, g), _fit(ctx, hist, g, waves=1), _fit(ctx, hist, g, waves=3), _fit(ctx, hist, g, waves=7),
                  _fit(ctx, Xp, g, rows=ROWS[perm], t_start=T_START[perm])]
        for o in others:
            for k in ('cp', 'support', 'H', 'b'):
                assert _bits(o[k], base[k]), (name, k)
            assert list(o['stats'][:4]) == list(base['stats'][:4]) and list(o['stats'][6:]) == list(base['stats'][6:])


def test_null_rows_and_start_times_are_the_full_and_zero_arrays(ctx, hist):
    for name, g in GRIDS.items():
        a = _fit(ctx, hist, g, rows=None, t_start=None)
        b = _fit(ctx, hist, g, rows=np.full(N_FORM, N_ROWS), t_start=np.zeros(N_FORM))
        c = _fit(ctx, hist, g, rows=np.full(N_FORM, N_ROWS + 50), t_start=np.zeros(N_FORM))       # clamped to n_rows
        for o in (b, c):
            for k in ('cp', 'support', 'H', 'b', 'stats'):
                assert _bits(o[k], a[k]), (name, k)


def test_no_sample_at_all_gives_the_prior(ctx, hist):
    for name, g in GRIDS.items():
        prior = np.empty((g.nt, 2, g.ny, g.nx))
        prior[:, 0], prior[:, 1] = 2.5, -1.25
        got = _fit(ctx, hist, g, rows=np.array([1, 0, 1]), prior=prior)
        assert list(got['stats'][:4]) == [0.0] * 4 and not got['H'].any() and not got['b'].any()
        assert np.array_equal(got['cp'], prior)
        assert got['stats'][4] == 0.0 and got['stats'][5] == 0.0


def test_refusals_launch_nothing(ctx, hist):
    """Every D2D_EINVAL of the header, raised as D2DError by the workspace query: nothing is launched."""
    import d2dhip
    import torch
    g = GRIDS['steady-5x6']
    dX = ctx.dev(hist)
    ok = dict(w_max=W_MAX, lam=LAM, mu=MU, cg_tol=CG_TOL, cg_max=100)
    bad_kw = [dict(w_max=0.0), dict(w_max=np.inf), dict(w_max=np.nan), dict(mu=0.0), dict(mu=-1.0), dict(mu=np.nan), dict(lam=(-1.0, 0.0, 0.0)),
              dict(lam=(0.0, np.inf, 0.0)), dict(lam=(0.0, 0.0, np.nan)), dict(cg_tol=0.0), dict(cg_tol=1.0), dict(cg_max=0), dict(waves=-1)]
    for kw in bad_kw:
        with pytest.raises(d2dhip.D2DError):
            ctx.wind_fit(dX, N_AC, DT, _grid_c(g), **dict(ok, **kw))
    for dt_row in (0.0, -0.05, np.nan, np.inf):
        with pytest.raises(d2dhip.D2DError):
            ctx.wind_fit(dX, N_AC, dt_row, _grid_c(g), **ok)
    for bad in (g._replace(nx=3), g._replace(ny=3), g._replace(nt=2), g._replace(nt=3), g._replace(hx=0.0), g._replace(hy=-1.0),
                g._replace(nt=4, ht=0.0), g._replace(nt=8, ny=23, nx=23)):                       # 4232 control points > 4096
        with pytest.raises(d2dhip.D2DError):
            ctx.wind_fit(dX, N_AC, DT, _grid_c(bad), **ok)
    with pytest.raises(d2dhip.D2DError):                                                         # n_rows < 2
        ctx.wind_fit(ctx.dev(hist[:1]), N_AC, DT, _grid_c(g), **ok)
    with pytest.raises(d2dhip.D2DError):                                                         # n_ac outside 1 .. 64
        ctx.wind_fit(ctx.zeros(2, 5, 130), 65, DT, _grid_c(g), **ok)
    # NULL pointers and the sample bound, on the C entry itself
    p = d2dhip.WindFitParams(N_FORM, N_AC, N_ROWS, 100, 0, 0, DT, W_MAX, 0.0, 0.0, 0.0, MU, CG_TOL)
    gc = _grid_c(g)
    import ctypes as C
    cp, work = ctx.empty(1, 2, g.ny, g.nx), ctx.empty(1 << 16)
    P = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    o = d2dhip.WindFitOut(None, None, None, None)
    lib = ctx.lib
    assert lib.d2d_wind_fit_workspace(C.byref(p), C.byref(gc)) > 0
    for args in ((None, C.byref(p), P(dX), None, None, C.byref(gc), P(cp), P(work), C.byref(o)),
                 (ctx.h, None, P(dX), None, None, C.byref(gc), P(cp), P(work), C.byref(o)),
                 (ctx.h, C.byref(p), None, None, None, C.byref(gc), P(cp), P(work), C.byref(o)),
                 (ctx.h, C.byref(p), P(dX), None, None, None, P(cp), P(work), C.byref(o)),
                 (ctx.h, C.byref(p), P(dX), None, None, C.byref(gc), None, P(work), C.byref(o)),
                 (ctx.h, C.byref(p), P(dX), None, None, C.byref(gc), P(cp), None, C.byref(o))):
        assert lib.d2d_wind_fit(*args) == -1
    big = d2dhip.WindFitParams(1 << 20, 64, 33, 100, 0, 0, DT, W_MAX, 0.0, 0.0, 0.0, MU, CG_TOL)   # 32 * 2^26 = 2^31 samples
    assert lib.d2d_wind_fit_workspace(C.byref(big), C.byref(gc)) == -1
    assert lib.d2d_wind_fit_workspace(None, C.byref(gc)) == -1 and lib.d2d_wind_fit_workspace(C.byref(p), None) == -1
    ctx.sync()
    assert torch.cuda.is_available()


def _recovery_flight(ctx, name, n_form=1, gust=None):
    F, grid, knots, lam = WF.recovery_case(name)
    c = np.tile(WF.RECOVERY_C, (n_form, 1)); X0 = np.tile(WF.recovery_x0(), (n_form, 1))
    planes = lambda a: np.ascontiguousarray(np.asarray(a, float).T)       # noqa: E731
    out = ctx.gvf_run(ctx.dev(planes(X0)), ctx.dev(planes(c)), ctx.dev(np.full(4 * n_form, WF.RECOVERY_R)), 4, WF.RECOVERY_STEPS,
                      WF.RECOVERY_DT, WF.RECOVERY_V, record=('X',), wind=F, **({} if gust is None else dict(gust=gust)))
    return F, grid, knots, lam, out


@pytest.mark.parametrize('name', ['shear', 'gust'])
def test_recovery_on_the_device(ctx, name):
    """Context.gvf_run(wind=F), then the estimator class on the flown history: the error against F at the flown midpoints is at most
    twice what tests/test_wind_fit_cpu.py recorded for the CPU plant (the factor covers the two plants' integrators differing in the
    last digits, not the estimator)."""
    from d2d.wind import WindEstimator
    F, grid, (x, y, t), lam, out = _recovery_flight(ctx, name)
    est = WindEstimator(x, y, t, lam=lam, mu=1e-6).fit(ctx, out['X'], 4, WF.RECOVERY_DT)
    ctx.sync()
    Xh = out['X'].cpu().numpy()
    ms = WF.measure(Xh, 4, WF.RECOVERY_DT, grid)
    err, _ = WF.recovery_error(est.cp.cpu().numpy(), grid, F, ms)
    st = est.stats_host()
    print(f'{name}: max|F^ - F| = {err:.3e} (CPU baseline {WF.RECOVERY_ERR[name]:.1e}), rms {est.rms}, {st["cg_iters"]:.0f} CG iterations')
    assert st['used'] == (WF.RECOVERY_STEPS - 1) * 4 and st['cg_resid'] <= 1e-10
    assert err <= 2.0 * WF.RECOVERY_ERR[name]
    # the estimate is a device field: the library samples it where the host spline does
    host = est.field()
    pts = np.stack([ms['px'][:, 0], ms['py'][:, 0]])
    w = ctx.wind_sample(est.device_field(ctx), ctx.dev(np.ascontiguousarray(ms['tm'][:, 0])), ctx.dev(np.ascontiguousarray(pts))).cpu().numpy()
    wn = ctx.wind_sample(est.negated_device_field(ctx), ctx.dev(np.ascontiguousarray(ms['tm'][:, 0])), ctx.dev(np.ascontiguousarray(pts))).cpu().numpy()
    hx, hy = host.sample_many(ms['tm'][:, 0], pts[0], pts[1])
    assert np.abs(w[0] - hx).max() <= 1e-12 and np.abs(w[1] - hy).max() <= 1e-12 and np.array_equal(wn, -w)


def test_residual_rms_is_the_gust_level(ctx):
    """Eight formations through wind_ref.shear and a nearly white gust of 0.5 m/s: the fit's residual RMS is the gust, within a factor 2."""
    from d2d.wind import GustModel, WindEstimator
    sigma = 0.5
    F, grid, (x, y, t), lam, out = _recovery_flight(ctx, 'shear', n_form=8, gust=GustModel(sigma, tau=0.1, seed=7))
    est = WindEstimator(x, y, t, lam=lam, mu=1e-6).fit(ctx, out['X'], 4, WF.RECOVERY_DT)
    rms = est.rms
    print(f'rms = {rms}, sigma = {sigma}')
    assert est.stats_host()['used'] > 0.9 * (WF.RECOVERY_STEPS - 1) * 32
    assert 0.5 * sigma <= rms[0] <= 2.0 * sigma and 0.5 * sigma <= rms[1] <= 2.0 * sigma
