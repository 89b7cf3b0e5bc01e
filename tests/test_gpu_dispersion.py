"""GPU: d2d_track_dispersion (ABI 128) against its CPU statement tests/dispersion_ref.py -- parity of every output on every launch
shape, independence of the batch layout, chaining through S_out / S_in, the reductions against torch, the refusals -- and against
the flight itself: the sample covariance of 4096 gust replicas flown by d2d_sim_track_run_gust.
Tolerance of the parity: TOL = 10 x dispersion_ref.CPU_FLOOR (what two CPU evaluations of the statement differ by), relative to the
largest diagonal entry of S at that row.  Measured on an MI355X: see DESIGN.md 5.27."""
import ctypes as C

import numpy as np
import pytest

import dispersion_ref as D
from oracle import sim as S

pytestmark = pytest.mark.gpu

DT = 0.05
TOL = 10.0 * D.CPU_FLOOR
N_MAX = 130
DIAG = [i * (i + 1) // 2 + i for i in range(D.NS)]
EINVAL = -1


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def _model(sigma=1.5, corr=0.0):
    from d2d.wind import GustModel
    return GustModel(sigma, tau=2.0, seed=5, form_corr=corr)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _tables(x, y, seed=11):
    """Per drone: eight fence edges round its path (rows 2 and 5 absent) and three discs beside it (row 1 absent)."""
    rng = np.random.default_rng(seed)
    n = x.shape[1]
    edges, discs = np.zeros((n, 8, 4)), np.zeros((n, 3, 3))
    for d in range(n):
        th = rng.uniform(0, 2 * np.pi) + np.arange(8) * (2 * np.pi / 8)
        a = np.stack([np.cos(th), np.sin(th)], 1)
        a /= np.hypot(a[:, 0], a[:, 1])[:, None]
        b = (a @ np.array([x[:, d], y[:, d]])).max(1) + rng.uniform(5.0, 40.0, 8)
        edges[d] = np.column_stack([a, b, np.full(8, 0.1)])
        edges[d, [2, 5]] = 0.0
        for m in range(3):
            ph = rng.uniform(0, 2 * np.pi)
            discs[d, m] = [x[0, d] + 150.0 * np.cos(ph), y[0, d] + 150.0 * np.sin(ph), 20.0 + 5.0 * m]
        discs[d, 1, 2] = 0.0
    return edges, discs


def _start_cov(n, seed=3):
    rng = np.random.default_rng(seed)
    S0 = np.zeros((28, n))
    for d in range(n):
        L = rng.normal(size=(7, 7)) * np.array([0.5, 0.5, 0.02, 0.02, 0.2, 1.0, 1.0])[:, None]
        S0[:, d] = D.pack(L @ L.T)
    return S0


def _device_derivatives(ctx, x, y, dt):
    """(4, T, n) = xd, yd, xdd, ydd as the existing tracking loop computes and records them (Yd_hist, Ydd_hist of d2d_sim_track_run:
    row q holds those of sample q + 1; row 0 of the result, which nothing uses, repeats row 1).  Two rows: the tracking loop takes none -- the one first
    difference, exact to an ulp whoever forms it."""
    T, n = x.shape
    if T < 3:
        return np.stack([np.stack(D.derivatives(x[:, d], y[:, d], dt)) for d in range(n)], 2)
    X0 = np.stack([x[0], y[0], np.zeros(n), np.zeros(n), np.full(n, 12.0)])
    out = ctx.track_run(ctx.dev(np.ascontiguousarray(x)), ctx.dev(np.ascontiguousarray(y)), ctx.dev(X0), dt, record=('Yd', 'Ydd'))
    ctx.sync()
    Yd, Ydd = out['Yd'].cpu().numpy(), out['Ydd'].cpu().numpy()
    der = np.zeros((4, T, n))
    der[0, 1:], der[1, 1:], der[2, 1:], der[3, 1:] = Yd[:T - 1, 0], Yd[:T - 1, 1], Ydd[:T - 1, 0], Ydd[:T - 1, 1]
    der[:, 0] = der[:, 1]
    return der


def _device_gains(ctx, x, y, dt, der):
    """K (T, n, 2, 5) of the existing d2d_ctrl_gain at X = Xr for every (row, drone), from the derivatives der: the statement then
    isolates the new code."""
    T, n = x.shape
    Y = np.zeros((8, T, n))
    Y[0], Y[1], Y[2:6] = x, y, der
    Yd = ctx.dev(np.ascontiguousarray(Y.reshape(8, T * n)))
    Xr, _, _, _ = ctx.ctrl_gain(ctx.zeros(5, T * n), Yd, dt=dt)
    _, dX, _, K = ctx.ctrl_gain(Xr, Yd, dt=dt)
    ctx.sync()
    assert float(dX.abs().max()) == 0.0
    return K.cpu().numpy().reshape(2, 5, T, n).transpose(2, 3, 0, 1)


_CACHE = {}


def _case(ctx, T, with_S):
    """The N_MAX references of T rows, their tables, the device's own gains and the statement of every drone -- computed once."""
    key = (T, with_S)
    if key not in _CACHE:
        x, y = D.references(N_MAX, T, DT)
        edges, discs = _tables(x, y)
        S0 = _start_cov(N_MAX) if with_S else None
        if ('K', T) not in _CACHE:
            der = _device_derivatives(ctx, x, y, DT)
            _CACHE[('K', T)] = (der, _device_gains(ctx, x, y, DT, der))
        der, K = _CACHE[('K', T)]
        k = _model().numbers(DT)
        ref = D.dispersion_batch(x, y, DT, k['a'], k['s'], k['sigma'], S0=S0, K=K, edges=edges, discs=discs, deriv=der)
        _CACHE[key] = (x, y, edges, discs, S0, ref)
    return _CACHE[key]


def _run(ctx, x, y, edges=None, discs=None, S0=None, dt=DT, model=None, record_P=True):
    out = ctx.track_dispersion(ctx.dev(np.ascontiguousarray(x)), ctx.dev(np.ascontiguousarray(y)), gust=model or _model(), dt=dt,
                               fence=None if edges is None else ctx.dev(np.ascontiguousarray(edges)),
                               keep_out=None if discs is None else ctx.dev(np.ascontiguousarray(discs)),
                               S0=None if S0 is None else ctx.dev(np.ascontiguousarray(S0)), record_P=record_P)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_extreme(name, d, got, got_row, rows_ref, tol_rows, largest):
    """got / got_row against the per-row reference values rows_ref (entry q: row q + 1) with per-row tolerances: the value within
    tolerance of the reference's extreme, the row equal unless the reference's value at the device's row ties within tolerance."""
    if not np.isfinite(rows_ref).any():                                       # +inf on every row: the first one
        assert np.isinf(got) and got_row == 1, (name, d, got, got_row)
        return 0.0
    q = int(np.argmax(rows_ref) if largest else np.argmin(rows_ref))
    err = abs(got - rows_ref[q])
    assert err <= tol_rows[q], (name, d, got, rows_ref[q], tol_rows[q])
    if got_row != q + 1:
        assert 1 <= got_row <= len(rows_ref) and abs(rows_ref[got_row - 1] - rows_ref[q]) <= tol_rows[q] + tol_rows[got_row - 1], (name, d, got_row, q + 1)
    return err / max(tol_rows[q], 1e-300)


# ---- 1. parity with the statement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_S', [False, True])
@pytest.mark.parametrize('T', [2, 3, 40])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 130])
def test_parity_with_the_statement(ctx, n, T, with_S):
    x, y, edges, discs, S0, ref = _case(ctx, T, with_S)
    got = _run(ctx, x[:, :n], y[:, :n], edges[:n], discs[:n], None if S0 is None else S0[:, :n])
    worst, worst_red = 0.0, 0.0
    for d in range(n):
        r = ref[d]
        hist = r['S_hist']
        diag = np.abs(hist[:, DIAG]).max(1)                                    # the largest diagonal entry of S at each row
        eP = np.abs(got['Ppos'][:, :, d] - r['Ppos']).max(1) / diag
        eS = np.abs(got['S'][:, d] - r['S']).max() / diag[-1]
        worst = max(worst, eP.max(), eS)
        assert eP.max() <= TOL and eS <= TOL, (d, eP.max(), eS)
        # the reductions: a variance along a unit vector is within 2 TOL diag of the statement's, its root and the ratios accordingly
        dvar = 2.0 * TOL * diag[1:]
        with np.errstate(divide='ignore', invalid='ignore'):
            tol_sn = lambda sn: np.where(sn > 0, dvar / (2.0 * sn), np.sqrt(dvar)) + 1e-15 * sn      # noqa: E731
            tol_k = lambda kk, sn: np.where(np.isfinite(kk), np.abs(kk) * (dvar / (2.0 * sn * sn) + 1e-13), 0.0)      # noqa: E731
            worst_red = max(worst_red, _check_extreme('sig_max', d, got['sig_max'][d], got['sig_row'][d], r['sig_rows'], tol_sn(r['sig_rows']), True))
            for e in range(edges.shape[1]):
                sn, kk = r['fence_sn_rows'][e], r['fence_k_rows'][e]
                absent = not edges[d, e, :2].any()
                if absent:
                    assert got['fence_sn'][e, d] == 0.0 and got['fence_k'][e, d] == np.inf and got['fence_row'][e, d] == -1
                    continue
                assert abs(got['fence_sn'][e, d] - sn.max()) <= tol_sn(sn)[np.argmax(sn)], (d, e)
                worst_red = max(worst_red, _check_extreme('fence_k', d, got['fence_k'][e, d], got['fence_row'][e, d], kk, tol_k(kk, sn), False))
            for m in range(discs.shape[1]):
                if not discs[d, m, 2] > 0:
                    assert got['disc_k'][m, d] == np.inf and got['disc_row'][m, d] == -1
                    continue
                kk, sn = r['disc_k_rows'][m], r['disc_sn_rows'][m]
                worst_red = max(worst_red, _check_extreme('disc_k', d, got['disc_k'][m, d], got['disc_row'][m, d], kk, tol_k(kk, sn), False))
    print(f'n={n} T={T} S_in={with_S}: largest relative error of Ppos / S {worst:.3e} (tolerance {TOL:.1e}); reductions at {worst_red:.3f} of theirs')


# ---- 2. layout independence and chaining -----------------------------------------------------------------------------------------
def test_a_drone_alone_gives_the_bytes_it_gives_in_the_batch(ctx):
    x, y, edges, discs, S0, _ = _case(ctx, 40, True)
    full = _run(ctx, x, y, edges, discs, S0)
    for d in (0, 1, 62, 64, 65, 129):                                          # every kind of reference, first and last lanes of a wave
        one = _run(ctx, x[:, d:d + 1], y[:, d:d + 1], edges[d:d + 1], discs[d:d + 1], S0[:, d:d + 1])
        for k, v in one.items():
            assert _bits(v[..., 0], full[k][..., d]), (d, k, np.abs(v[..., 0] - full[k][..., d]).max())


def _dyadic_references(n, T):
    """References whose derivatives are exact in fp64 whatever rows a call sees: quadratics in the row index with dyadic coefficients on
    a dyadic step (second-order edge formulas are exact on quadratics), ~14 m/s with ~1 m/s^2 of acceleration -- turning and changing
    speed, all different."""
    rng = np.random.default_rng(21)
    i = np.arange(T, dtype=float)[:, None]
    c1x, c1y = rng.integers(36, 56, n) / 64.0, rng.integers(-40, 41, n) / 64.0
    c2x, c2y = rng.integers(-4, 5, n) / 1024.0, rng.integers(-4, 5, n) / 1024.0
    return rng.integers(-64, 64, n) + c1x * i + c2x * i * i, rng.integers(-64, 64, n) + c1y * i + c2y * i * i


def test_chaining_through_S_out_and_S_in_gives_the_bytes_of_one_call(ctx):
    dt, n = 0.0625, 65
    x, y = _dyadic_references(n, 41)
    whole = _run(ctx, x, y, dt=dt)
    first = _run(ctx, x[:21], y[:21], dt=dt)
    second = _run(ctx, x[20:], y[20:], S0=first['S'], dt=dt)
    assert _bits(first['Ppos'], whole['Ppos'][:21]) and _bits(second['Ppos'], whole['Ppos'][20:]) and _bits(second['S'], whole['S'])
    assert np.abs(whole['S'] - first['S']).max() > 0 and len(np.unique(whole['S'][0])) > n // 2          # (they evolve, and differ per drone)


# ---- 3. the reductions --------------------------------------------------------------------------------------------------------------
def test_reductions_equal_torch_on_the_recorded_covariances(ctx):
    import torch
    T, n = 40, 130
    x, y, edges, discs, _, _ = _case(ctx, T, False)
    xr, yr, ed, dc = (ctx.dev(np.ascontiguousarray(a)) for a in (x, y, edges, discs))
    out = ctx.track_dispersion(xr, yr, gust=_model(), dt=DT, fence=ed, keep_out=dc, record_P=True)
    ctx.sync()
    P = out['Ppos'][1:]                                                        # [T - 1][3][n]
    xx, xy, yy = P[:, 0], P[:, 1], P[:, 2]
    px, py = xr[1:], yr[1:]
    inf = torch.tensor(float('inf'), dtype=torch.float64, device=xr.device)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300))[torch.isfinite(b)].max())      # noqa: E731
    worst = 0.0
    for e in range(8):
        ax, ay, b = ed[:, e, 0], ed[:, e, 1], ed[:, e, 2]
        sn = (ax * ax * xx + 2 * ax * ay * xy + ay * ay * yy).clamp_min(0).sqrt()
        if not edges[0, e, :2].any():
            assert (out['fence_sn'][e] == 0).all() and torch.isinf(out['fence_k'][e]).all() and (out['fence_row'][e] == -1).all()
            continue
        kk = torch.where(sn > 0, (b - (ax * px + ay * py)) / sn, inf)
        worst = max(worst, rel(out['fence_sn'][e], sn.max(0).values), rel(out['fence_k'][e], kk.min(0).values))
        at = kk.gather(0, (out['fence_row'][e].long() - 1)[None])[0]           # the device's row holds the minimum
        worst = max(worst, rel(at, kk.min(0).values))
    for m in range(3):
        if not discs[0, m, 2] > 0:
            assert torch.isinf(out['disc_k'][m]).all() and (out['disc_row'][m] == -1).all()
            continue
        rx, ry = px - dc[:, m, 0], py - dc[:, m, 1]
        dist = (rx * rx + ry * ry).sqrt()
        ux, uy = rx / dist, ry / dist
        sn = (ux * ux * xx + 2 * ux * uy * xy + uy * uy * yy).clamp_min(0).sqrt()
        kk = torch.where(sn > 0, (dist - dc[:, m, 2]) / sn, inf)
        worst = max(worst, rel(out['disc_k'][m], kk.min(0).values))
        worst = max(worst, rel(kk.gather(0, (out['disc_row'][m].long() - 1)[None])[0], kk.min(0).values))
    hd = 0.5 * (xx - yy)
    sg = (0.5 * (xx + yy) + (hd * hd + xy * xy).sqrt()).clamp_min(0).sqrt()
    worst = max(worst, rel(out['sig_max'], sg.max(0).values))
    print('reductions against torch on Ppos_hist: largest relative difference', worst)
    assert worst <= 1e-12
    # absent rows change nothing: the six present edges and the two present discs alone give the same bytes
    keep_e, keep_d = [0, 1, 3, 4, 6, 7], [0, 2]
    a = {k: v.cpu().numpy() for k, v in out.items()}
    b = _run(ctx, x, y, edges[:, keep_e], discs[:, keep_d])
    for k in ('S', 'Ppos', 'sig_max', 'sig_row'):
        assert _bits(a[k], b[k]), k
    for k in ('fence_sn', 'fence_k', 'fence_row'):
        assert _bits(a[k][keep_e], b[k]), k
    for k in ('disc_k', 'disc_row'):
        assert _bits(a[k][keep_d], b[k]), k
    # ... and sigma = 0: no dispersion at all, every k +inf
    z = _run(ctx, x[:, :5], y[:, :5], edges[:5], discs[:5], model=_model(0.0))
    assert not z['S'].any() and not z['Ppos'].any() and not z['sig_max'].any() and np.isinf(z['fence_k']).all() and np.isinf(z['disc_k']).all()


# ---- 4. against the flight ----------------------------------------------------------------------------------------------------------
def test_prediction_against_the_sample_covariance_of_flown_gust_replicas(ctx):
    """One S-turn at 15 m/s over 12 s; R = 4096 replicas (n_ac = 1, form_corr = 0, tau = 2 s) through d2d_sim_track_run_gust and one
    gust-free flight.  sigma = 0.2 m/s, not 0.3: the statement predicts a standard deviation of v - v_r of 0.78 sigma, and at 0.3 the
    err_sats bound of 1 m/s is 4.3 of them away -- over 4096 x 240 samples some replica would touch it (six CPU replicas through
    tests/gust_ref.py touched none even at 0.3; on an MI355X at 0.2 the largest |dX| / err_sats of all replicas and rows is 0.66).  At the middle and the last row the second moments of (x, y) about the
    gust-free flight lie within five standard errors of the prediction; the statement with K = 0, with Ed = 0 and with cont_jac's
    quirk entries in A must each fall outside that band at the last row."""
    import torch
    R, T, sigma = 4096, 241, 0.2
    t = np.arange(T) * DT
    x, y = D.s_turn(t, 15.0, 0.6, 12.0)
    gm = _model(sigma)
    k = gm.numbers(DT)
    X0 = D.reference_states(x, y, DT)[1]                                       # the state of the first reference sample the loop uses
    xr, yr = ctx.dev(np.ascontiguousarray(np.tile(x[:, None], (1, R)))), ctx.dev(np.ascontiguousarray(np.tile(y[:, None], (1, R))))
    fl = ctx.track_run(xr, yr, ctx.dev(np.ascontiguousarray(np.tile(X0[:, None], (1, R)))), DT, record=('X', 'U', 'dX'), gust=gm, gust_n_ac=1)
    free = ctx.track_run(xr[:, :1].contiguous(), yr[:, :1].contiguous(), ctx.dev(np.ascontiguousarray(X0[:, None])), DT, record=('X',))
    pred = ctx.track_dispersion(xr[:, :1].contiguous(), yr[:, :1].contiguous(), gust=gm, dt=DT, record_P=True)
    ctx.sync()
    # the condition: no replica touches a saturation at any row (dX is the clipped error, U the clipped command)
    dX, U = fl['dX'][:T - 1], fl['U'][:T - 1]
    sats = torch.tensor(S.ERR_SATS, dtype=torch.float64, device=dX.device)[None, :, None]
    frac = float((dX.abs() / sats).max())
    print('largest |dX| / err_sats', frac, '|U_phi| max', float(U[:, 0].abs().max()), 'U_v range', float(U[:, 1].min()), float(U[:, 1].max()))
    assert frac < 1.0 and float(U[:, 0].abs().max()) < S.PHI_LIM and S.V_MIN < float(U[:, 1].min()) and float(U[:, 1].max()) < S.V_MAX
    dev = (fl['X'][:, :2] - free['X'][:, :2]).cpu().numpy()                   # [T][2][R]
    P = pred['Ppos'].cpu().numpy()[:, :, 0]
    Kdev = _device_gains(ctx, x[:, None], y[:, None], DT, np.stack(D.derivatives(x, y, DT))[:, :, None])[:, 0]
    variants = {'K = 0': dict(K=np.zeros_like(Kdev)), 'Ed = 0': dict(K=Kdev, no_gust_input=True), 'quirk A': dict(K=Kdev, quirk=True)}

    def inside(Pp, m):
        """are xx, xy, yy of Pp within five standard errors (taken at Pp) of the sample moments m"""
        xx, xy, yy = Pp
        se = np.sqrt(2.0 / (R - 1))
        return (abs(m[0] - xx) <= 5 * se * xx and abs(m[2] - yy) <= 5 * se * yy and abs(m[1] - xy) <= 5 * np.sqrt((xx * yy + xy * xy) / (R - 1)))

    for row in (T // 2, T - 1):
        m = np.array([(dev[row, 0] ** 2).mean(), (dev[row, 0] * dev[row, 1]).mean(), (dev[row, 1] ** 2).mean()])
        print(f'row {row}: sample xx, xy, yy = {m}, predicted {P[row]}, ratios {m[0] / P[row, 0]:.4f} {m[2] / P[row, 2]:.4f}, '
              f'xy difference {m[1] - P[row, 1]:+.3e} of allowed {5 * np.sqrt((P[row, 0] * P[row, 2] + P[row, 1] ** 2) / (R - 1)):.3e}')
        assert inside(P[row], m), (row, m, P[row])
    for name, kw in variants.items():
        v = D.dispersion(x, y, DT, k['a'], k['s'], k['sigma'], **kw)['Ppos'][T - 1]
        print(f'variant {name}: predicted {v} at the last row')
        assert not inside(v, m), (name, v, m)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_before_a_launch_and_the_host_refuses_by_name(ctx):
    import d2dhip
    import full_sim as FS
    from d2d.wind import SplineWindField
    canary = ctx.dev(np.full(4096, 12345.0))
    res = D.entry_point_refusals(ctx.lib, ctx.h, C.c_void_p(canary.data_ptr()))
    ctx.sync()
    assert len(res) >= 20 and all(rc == EINVAL for _, rc in res), res
    assert bool((canary == 12345.0).all())                                    # nothing was written: no kernel ran
    t, z = np.arange(5) * DT, np.zeros((5, 2))
    with pytest.raises(NotImplementedError, match='SplineWindField'):
        FS.track_dispersion(t, z, z, (0., 0.), _model(), windfield=SplineWindField.__new__(SplineWindField))
    with pytest.raises(NotImplementedError, match='GVF'):
        FS.track_dispersion(t, z, z, (0., 0.), _model(), loop='gvf')
    with pytest.raises(NotImplementedError, match='dfff_run'):
        FS.track_dispersion(t, z, z, (0., 0.), _model(), loop='dfff')
    with pytest.raises(NotImplementedError, match='form_corr'):
        FS.dispersion_margin(dict(gust=_model(corr=0.3), sig_max=np.ones(2)), 1.35e-3, pair=(0, 1))
    with pytest.raises(ValueError, match='rows per drone'):
        ctx.track_dispersion(ctx.zeros(5, 2), ctx.zeros(5, 2), gust=_model(), dt=DT, fence=np.zeros((d2dhip.MAX_FENCE + 1, 4)))


def test_full_sim_report_and_margin_follow_the_context_call(ctx):
    """full_sim.track_dispersion is Context.track_dispersion with implement_controller_batch's constants; dispersion_margin scales it."""
    import full_sim as FS
    from d2d.opty_utils import GeoFence
    T, n = 40, 5
    x, y, _, _, _, _ = _case(ctx, T, False)
    x, y = x[:, :n], y[:, :n]
    fence = GeoFence([(-400., -400.), (400., -400.), (400., 400.), (-400., 400.)], margin=2.0)
    rep = FS.track_dispersion(np.arange(T) * DT, x, y, (0., 0.), _model(), fence=fence)
    dctx = FS.d2dhip.default_context()
    dctx.sync()
    edges = np.broadcast_to(fence.lowered()[None], (n, 4, 4))
    got = _run(ctx, x, y, edges)
    for k in ('S', 'sig_max', 'fence_sn', 'fence_k', 'fence_row'):
        assert _bits(rep[k].cpu().numpy(), got[k]), k
    m = FS.dispersion_margin(rep, 1.35e-3)
    assert abs(m['z'] - 3.0) < 2e-3 and 'pair' not in m
    assert np.allclose(m['fence'].cpu().numpy(), m['z'] * got['fence_sn'], rtol=1e-15, atol=0.0)
    assert np.allclose(m['disc'].cpu().numpy(), m['z'] * got['sig_max'], rtol=1e-15, atol=0.0)
    mp = FS.dispersion_margin(rep, 1.35e-3, pair=(0, 1))
    assert np.isclose(float(mp['pair']), m['z'] * np.hypot(got['sig_max'][0], got['sig_max'][1]))
