"""GPU parity of the flight audit (d2d_flight_audit, csrc/audit_kernels.hip) with its CPU statement tests/flight_audit_ref.py on small
synthetic histories (coordinates within +-1e3 m), its bit-identity across block lengths, its tie rules and refusals, and the audits
that the GVF loop, the tracking loop and the mission chain hand back.

Tolerances: distances, clearances, errors and the envelope 1e-10 (m, rad, m/s) absolute -- about twenty fp64 roundings of quantities
<= 1e3 allow 1e-12, two orders are left for contraction and sqrt; partner indices and counts equal, on inputs the CPU statement
shows to be 1e-6 m away from every decision; a reported time gives the reported minimum within 1e-10 when the statement's distance
function is evaluated there, and equals the statement's time within 1e-9 dt_row where the relative motion of that segment is >= 1 m."""
import ctypes as C

import numpy as np
import pytest

import flight_audit_ref as FA

pytestmark = pytest.mark.gpu
TOL = 1e-10
FLOATS = ('sep_dist', 'stat_clear', 'mov_clear', 'err_max', 'phi_max', 'v_min', 'v_max')
TIMES = ('sep_time', 'stat_time', 'mov_time', 'err_time')
INTS = ('sep_partner', 'sep_count', 'stat_count', 'mov_count', 'err_count', 'status')
WORST = {}          # the largest differences seen so far, printed by the parity test (pytest -s): the figures of DESIGN 5.15


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    return d2dhip.default_context()


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _run(ctx, X, n_ac, dt, **kw):
    import torch
    dev = {k: (ctx.dev(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    if isinstance(dev.get('rows'), torch.Tensor):
        dev['rows'] = dev['rows'].to(torch.int32)
    out = ctx.flight_audit(ctx.dev(np.ascontiguousarray(X)), n_ac, dt, **dev)
    ctx.sync()
    return _np(out)


def _same(a, b):
    """Equal values with NaN = NaN and inf = inf."""
    return np.array_equal(a, b, equal_nan=True)


def _compare(got, X, n_ac, dt, what='', check_margins=True, **kw):
    """The device's dictionary against the CPU statement on the same inputs (the moving centres: the library's own)."""
    kw = {k: v for k, v in kw.items() if k != 'rows_per_block'}
    mg = {}
    ref = FA.audit(X, n_ac, dt, centres=got.get('mov_work'), margins=mg, **kw)
    assert not check_margins or (mg['count'] > 1e-6 and mg['partner'] > 1e-6), (what, mg)       # no decision within 1e-6 m of turning
    for k in INTS:
        if k in ref:
            assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    for k in FLOATS:
        if k in ref:
            fin = np.isfinite(ref[k])
            assert _same(got[k][~fin], ref[k][~fin]), (what, k)
            err = float(np.abs(got[k][fin] - ref[k][fin]).max(initial=0.0))
            WORST[k] = max(WORST.get(k, 0.0), err)
            assert err <= TOL, (what, k, err)
    n_rows, _, N = X.shape
    n_form = N // n_ac
    t0 = np.broadcast_to(np.asarray(kw.get('t_start', 0.0) if kw.get('t_start') is not None else 0.0, dtype=np.float64), (n_form,))
    rows = np.full(n_form, n_rows) if kw.get('rows') is None else np.clip(kw['rows'], 0, n_rows)
    for k in TIMES:
        if k not in ref:
            continue
        g, r = np.atleast_2d(got[k]), np.atleast_2d(ref[k])
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, k)
        for m, d in zip(*np.nonzero(~np.isnan(r))):
            f = d // n_ac
            t, win = g[m, d], (t0[f], t0[f] + (rows[f] - 1) * dt)
            assert win[0] - 1e-12 <= t <= win[1] + 1e-9 * dt, (what, k, t, win)
            if k == 'err_time':
                assert abs(t - r[m, d]) <= 1e-9 * dt
                continue
            # the statement's distance function at the device's time gives the device's minimum
            if k == 'sep_time':
                P = X[:, :2, f * n_ac + got['sep_partner'][d]] - X[:, :2, d]
                val, rep = FA.pair_distance(X, n_ac, dt, d, got['sep_partner'][d], t, t0[f], rows[f]), got['sep_dist'][d]
            else:
                ctr = kw['static'][f, m, :2] if k == 'stat_time' else got['mov_work'][f, m]
                rad = kw['static'][f, m, 2] if k == 'stat_time' else kw['disc'][f, m, 0]
                P = X[:, :2, d] - (ctr if ctr.ndim == 1 else ctr.T)
                val, rep = FA.disc_clearance(X, dt, d, ctr, rad, t, t0[f], rows[f]), np.atleast_2d(got[k.replace('time', 'clear')])[m, d]
            WORST['at ' + k] = max(WORST.get('at ' + k, 0.0), abs(val - rep))
            assert abs(val - rep) <= TOL, (what, k, d, val, rep)
            i = min(int(np.floor((r[m, d] - t0[f]) / dt + 1e-9)), rows[f] - 2)
            if i >= 0 and np.hypot(*(P[i + 1] - P[i])) >= 1.0:       # s* is well conditioned
                WORST[k] = max(WORST.get(k, 0.0), abs(t - r[m, d]) / dt)
                assert abs(t - r[m, d]) <= 1e-9 * dt, (what, k, d, t, r[m, d])
    return ref


def _tables(n_form, n_rows, dt, t0, seed):
    """Static discs (an absent one in the middle) and two moving discs with 4 knots (one absent for odd formations)."""
    rng = np.random.default_rng(seed)
    static = np.concatenate([rng.uniform(-60, 60, (n_form, 3, 2)), rng.uniform(2, 25, (n_form, 3, 1))], 2)
    static[:, 1, 2] = np.where(np.arange(n_form) % 2 == 0, -1.0, 0.0)
    tk = t0[:, None, None] + np.cumsum(rng.uniform(0.3, 1.0, (n_form, 2, 4)) * max(n_rows, 2) * dt * 0.4, axis=2) - 0.3 * n_rows * dt
    knots = np.concatenate([tk[..., None], rng.uniform(-60, 60, (n_form, 2, 4, 2))], 3)
    disc = np.stack([rng.uniform(2, 20, (n_form, 2)), rng.integers(0, 2, (n_form, 2)).astype(float)], 2)
    disc[1::2, 1, 0] = 0.0
    return static, knots, disc


SHAPES = [(1, 1), (1, 2), (3, 3), (13, 5), (2, 8), (2, 64), (22, 3)]


@pytest.mark.parametrize('n_rows', [1, 2, 3, 33])
@pytest.mark.parametrize('n_form,n_ac', SHAPES)
def test_parity_with_the_cpu_statement(ctx, n_form, n_ac, n_rows):
    dt = 0.5
    seed = 1000 * n_form + 10 * n_ac + n_rows
    X = FA.synthetic_history(n_form, n_ac, n_rows, seed, span=60.0 if n_ac < 64 else 400.0)
    # bare: the history alone
    _compare(_run(ctx, X, n_ac, dt), X, n_ac, dt, 'bare')
    # everything: valid rows (0, 1 and n_rows among them) with the unread rows NaN, start times, references, discs
    rng = np.random.default_rng(seed + 1)
    rows = rng.integers(0, n_rows + 1, n_form)
    rows[:3] = [n_rows, 1, 0][:min(3, n_form)]
    t0 = rng.uniform(0.0, 50.0, n_form)
    Xn = X.copy()
    for f in range(n_form):
        Xn[rows[f]:, :, f * n_ac:(f + 1) * n_ac] = np.nan
    x_ref = np.where(np.isnan(Xn[:, 0]), np.nan, Xn[:, 0] + rng.uniform(-2, 2, Xn[:, 0].shape))
    y_ref = np.where(np.isnan(Xn[:, 1]), np.nan, Xn[:, 1] + rng.uniform(-2, 2, Xn[:, 1].shape))
    static, knots, disc = _tables(n_form, n_rows, dt, t0, seed + 2)
    kw = dict(rows=rows, t_start=t0, x_ref=x_ref, y_ref=y_ref, static=static, knots=knots, disc=disc, d_safe=25.0, err_tol=1.5)
    got = _run(ctx, Xn, n_ac, dt, **kw)
    assert (got['status'] == 0).all()                # a refusal here: a row behind rows[f] was read
    _compare(got, Xn, n_ac, dt, 'all', **kw)
    # start times and discs without rows or references
    kw = dict(t_start=t0, static=static, d_safe=25.0)
    _compare(_run(ctx, X, n_ac, dt, **kw), X, n_ac, dt, 'static', **kw)
    print('largest |device - statement| so far:', {k: float('%.3g' % v) for k, v in sorted(WORST.items())})


def _closing(n_rows=33, at=15.5, n_form=3):
    """Formations of three: aircraft 0 and 1 pass each other on opposite courses 0.25 m apart, abeam exactly at row `at`; aircraft 2
    is far away; the formations differ by a shift and a speed.  Every coordinate is a binary fraction: s* and the time are exact."""
    X = np.zeros((n_rows, 5, 3 * n_form))
    i = np.arange(n_rows) - at
    for f in range(n_form):
        v = 2.0 + f
        X[:, 0, 3 * f], X[:, 1, 3 * f] = v * i + 10 * f, 5.0 * f
        X[:, 0, 3 * f + 1], X[:, 1, 3 * f + 1] = -v * i + 10 * f, 5.0 * f + 0.25
        X[:, 0, 3 * f + 2], X[:, 1, 3 * f + 2] = 300.0 + i, -200.0 + 7 * f
    X[:, 3] = 0.01 * np.arange(n_rows)[:, None]
    X[:, 4] = 12.0 + 0.1 * np.arange(n_rows)[:, None]
    return X


@pytest.mark.parametrize('at', [15.5, 16.0])
def test_block_boundaries(ctx, at):
    """The closest approach inside the segment 15 -> 16, and exactly at row 16: every block length gives the same bits."""
    X, dt = _closing(at=at), 0.5
    t0 = np.array([0.0, 3.0, 7.0])
    static = np.tile(np.array([[[4.0, 3.0, 1.0]]]), (3, 1, 1))
    knots = np.tile(np.array([[[[-5.0, -30.0, 2.0], [40.0, 60.0, 2.5]]]]), (3, 1, 1, 1)); disc = np.tile(np.array([[[1.5, 0.0]]]), (3, 1, 1))
    kw = dict(t_start=t0, static=static, knots=knots, disc=disc, x_ref=X[:, 0] + 0.5 + 0.01 * np.arange(33)[:, None], y_ref=X[:, 1] - 0.25, d_safe=3.0,
              err_tol=0.1)
    outs = [_run(ctx, X, 3, dt, rows_per_block=b, **kw) for b in (0, 1, 2, 16, 17, 33, 64, 0)]
    for o in outs[1:]:
        for k in outs[0]:
            assert _same(o[k], outs[0][k]) and o[k].tobytes() == outs[0][k].tobytes(), k
    ref = _compare(outs[0], X, 3, dt, **kw)
    expect = t0 + at * dt
    assert np.array_equal(ref['sep_time'][0::3], expect) and np.array_equal(outs[0]['sep_time'][1::3], expect)
    assert (outs[0]['sep_dist'].reshape(3, 3)[:, :2] == 0.25).all() and (outs[0]['sep_partner'].reshape(3, 3)[:, :2] == [1, 0]).all()


def test_tunnelling(ctx):
    """Two aircraft cross at right angles and meet between two rows: the audit sees it, the rows do not."""
    import torch
    n_rows, dt, step = 5, 0.1, 3.0
    i = np.arange(n_rows) - 2.5
    X = np.zeros((n_rows, 5, 2))
    X[:, 0, 0] = step * i
    X[:, 1, 1] = step * i
    got = _run(ctx, X, 2, dt)
    assert (got['sep_dist'] < 1e-10).all() and list(got['sep_partner']) == [1, 0] and np.abs(got['sep_time'] - 2.5 * dt).max() <= 1e-12
    Xd = ctx.dev(X)
    rowwise = torch.hypot(Xd[:, 0, 0] - Xd[:, 0, 1], Xd[:, 1, 0] - Xd[:, 1, 1]).min().item()
    assert rowwise > 1.0 and abs(rowwise - step / np.sqrt(2)) <= 1e-12


def test_ties(ctx):
    X = np.zeros((3, 5, 3))
    X[:, 0, 0] = [-1.0, 0.5, 2.0]                    # the closest approach to both partners inside the segment 0 -> 1, at the same s
    X[:, 1, 1], X[:, 1, 2] = 2.0, -2.0
    got = _run(ctx, X, 3, 1.0)
    assert got['sep_partner'][0] == 1 and got['sep_dist'][0] == 2.0 and abs(got['sep_time'][0] - 2.0 / 3.0) <= 1e-15
    Y = np.zeros((5, 5, 2))
    Y[:, 0, 1] = [3.0, 1.0, 3.0, 1.0, 3.0]
    for b in (0, 1, 2):
        got = _run(ctx, Y, 2, 0.5, rows_per_block=b)
        assert (got['sep_dist'] == 1.0).all() and (got['sep_time'] == 0.5).all()


def _refused(got, n_ac, f, bit):
    sl = slice(f * n_ac, (f + 1) * n_ac)
    assert got['status'][f] == bit and (np.delete(got['status'], f) == 0).all()
    for k, v in got.items():
        if k in ('status', 'mov_work'):
            continue
        assert (np.isnan(v[..., sl]) if v.dtype == np.float64 else v[..., sl] == -1).all(), k


def test_refusals(ctx):
    import d2dhip
    n_form, n_ac, n_rows, dt = 4, 3, 9, 0.5
    X = FA.synthetic_history(n_form, n_ac, n_rows, 5)
    t0 = np.array([0.0, 2.0, 4.0, 6.0])
    static, knots, disc = _tables(n_form, n_rows, dt, t0, 6)
    kw = dict(t_start=t0, static=static, knots=knots, disc=disc, x_ref=X[:, 0] + 1.0, y_ref=X[:, 1] + 1.0, d_safe=20.0, err_tol=0.5)
    # a NaN in one aircraft of one formation
    Xb = X.copy(); Xb[7, 4, 2 * n_ac + 1] = np.nan
    got = _run(ctx, Xb, n_ac, dt, **kw)
    _refused(got, n_ac, 2, d2dhip.AUDIT_NONFINITE)
    _compare(got, Xb, n_ac, dt, **kw)
    # a start time that is not finite, with moving discs
    tb = t0.copy(); tb[1] = np.inf
    kwb = dict(kw, t_start=tb)
    got = _run(ctx, X, n_ac, dt, **kwb)
    _refused(got, n_ac, 1, d2dhip.AUDIT_BAD_TSTART)
    _compare(got, X, n_ac, dt, **kwb)
    # a track whose knot times do not increase
    kb = knots.copy(); kb[3, 1, 2, 0] = kb[3, 1, 1, 0]
    kwb = dict(kw, knots=kb)
    got = _run(ctx, X, n_ac, dt, **kwb)
    _refused(got, n_ac, 3, d2dhip.AUDIT_BAD_TRACK)
    _compare(got, X, n_ac, dt, **kwb)


def test_einval_before_any_launch(ctx):
    import d2dhip
    import torch
    lib = ctx.lib
    N, n_rows = 6, 4
    X = ctx.zeros(n_rows, 5, N); t0 = ctx.zeros(2); ref = ctx.zeros(n_rows, N)
    static = ctx.zeros(2, 1, 3); knots = ctx.dev(np.tile(np.array([[0.0, 0, 0], [1.0, 1, 1]]), (2, 1, 1, 1))); disc = ctx.zeros(2, 1, 2)
    work = ctx.zeros(1 << 16); mov_work = ctx.zeros(2, 1, 2, n_rows)
    outs = {k: torch.full((64,), 7, dtype=torch.int32 if k in ('sep_partner', 'sep_count', 'stat_count', 'mov_count', 'err_count', 'status')
                          else torch.float64, device=ctx.device) for k in d2dhip.AUDIT_OUT}
    o = d2dhip.AuditOut(**{k: v.data_ptr() for k, v in outs.items()})
    ptr = d2dhip._ptr

    def call(p=None, X_=X, t_=t0, xr=ref, yr=ref, st=static, kn=knots, dc=disc, n_mov=1, n_knot=2, mw=mov_work):
        p = p or {}
        pp = d2dhip.AuditParams(p.get('n_form', 2), p.get('n_ac', 3), p.get('n_rows', n_rows), p.get('rpb', 0), p.get('n_stat', 1), 0,
                                p.get('dt_row', 0.5), 0.0, float('inf'))
        m = d2dhip.MovingObstaclesC(n_mov, n_knot, None if kn is None else kn.data_ptr(), None if dc is None else dc.data_ptr())
        return lib.d2d_flight_audit(ctx.h, C.byref(pp), ptr(X_), None, ptr(t_), ptr(xr), ptr(yr), ptr(st), C.byref(m), ptr(mw), ptr(work), C.byref(o))

    assert call() == 0
    ctx.sync()
    for v in outs.values():
        v.fill_(7)
    bad = [dict(X_=None), dict(p=dict(n_ac=0)), dict(p=dict(n_ac=65)), dict(p=dict(n_rows=0)), dict(p=dict(dt_row=0.0)),
           dict(p=dict(dt_row=float('nan'))), dict(p=dict(n_stat=-1)), dict(p=dict(n_stat=d2dhip.MAX_OBS + 1)), dict(n_mov=-1),
           dict(n_mov=d2dhip.MAX_MOV + 1), dict(st=None), dict(kn=None), dict(dc=None), dict(mw=None), dict(xr=None), dict(yr=None),
           dict(t_=None), dict(n_knot=1), dict(p=dict(rpb=-1))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.d2d_last_error()
    ctx.sync()
    assert all(bool((v == 7).all()) for v in outs.values())          # nothing was launched
    with pytest.raises(d2dhip.D2DError):
        ctx.flight_audit(X, 3, 0.5, x_ref=ref)
    with pytest.raises(d2dhip.D2DError):
        ctx.flight_audit(X, 3, 0.5, knots=knots, disc=disc)


def test_moving_centres_are_mov_sample_bit_for_bit(ctx):
    """The centre planes the audit used are mov_sample's, and a clearance whose minimum is AT a row is computed from that row's
    centre bit for bit.  Each disc runs along the aircraft's own y towards the stationary aircraft and turns back at a knot that a row
    hits (all times binary fractions): the closest approach is that row; with the y difference exactly 0 the distance is
    sqrt(fl(qx^2)) = |qx| exactly, so one ulp of the centre would show."""
    n_rows, dt, t0 = 12, 0.25, np.array([1.5, 20.0])
    X = np.zeros((n_rows, 5, 2))
    X[:, 0, :] = 3.0
    X[:, 1, 0], X[:, 1, 1] = 0.9, 0.7
    knots = np.array([[[[0.0, -7.3, 0.9], [1.5 + 5 * dt, 0.4, 0.9], [9.0, -11.7, 0.9]]],
                      [[[15.0, -9.1, 0.7], [20.0 + 7 * dt, 1.3, 0.7], [40.0, -30.0, 0.7]]]])
    disc = np.array([[[0.5, 0.0]], [[0.25, 1.0]]])
    got = _run(ctx, X, 1, dt, t_start=t0, knots=knots, disc=disc)
    ctr = ctx.mov_sample(ctx.dev(knots), ctx.dev(disc), ctx.dev(t0), n_rows, dt).cpu().numpy()
    assert got['mov_work'].tobytes() == ctr.tobytes()
    for d, row in ((0, 5), (1, 7)):
        assert ctr[d, 0, 1, row] == X[row, 1, d] and ctr[d, 0, 0, row] == knots[d, 0, 1, 1]       # the knot itself, abeam in y exactly
        dist = np.abs(X[:, 0, d] - ctr[d, 0, 0])
        assert int(np.argmin(dist)) == row and (np.delete(dist, row) > dist[row] + 0.1).all()
        assert got['mov_clear'][0, d] == dist[row] - disc[d, 0, 0]
        assert got['mov_time'][0, d] == t0[d] + row * dt
        assert got['mov_count'][0, d] == 0


@pytest.mark.parametrize('rec_stride', [1, 3])
def test_gvf_history(ctx, rec_stride):
    """A 4-aircraft GVF run of 41 rows whose stop rule fires, through CircularFormationGVF_batch(audit=...)."""
    import full_sim as fs
    from oracle import sim as S
    c = np.array([[0, -20], [25, -40], [25, -80], [0, -100.0]])
    X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (4, 1))
    X0[:, 0] += [0.0, 9.0, 21.0, 36.0]; X0[:, 1] += [0.0, -7.0, 5.0, -12.0]       # distinct poses: no partner ties
    Xo, *_ = S.formation_gvf_run(c, 60.0, 15.0, X0, 41, 0.05)
    X0f = np.stack([Xo[25], Xo[25] + 50.0])[:, :, :3]               # formation 0 stops where the oracle is at row 25, formation 1 never
    disc = [[22.0, 12.0, 4.0]]
    out = fs.CircularFormationGVF_batch(np.stack([c, c]), 60.0, 15.0, 4, X0f=X0f, t_start=2.0, t_step=0.05, t_end=2.0 + 40.5 * 0.05,
                                        X0=np.stack([X0, X0]), rec_stride=rec_stride, audit=dict(d_safe=12.0, static=disc))
    ctx.sync()
    stop = out['stop_row'].cpu().numpy()
    assert stop[0] < 41 <= stop[1]
    rows = -(-np.minimum(stop, 41) // rec_stride)
    X = out['X'].cpu().numpy()
    assert X.shape[0] == -(-41 // rec_stride)
    Xn = X.copy(); Xn[rows[0]:, :, :4] = np.nan                      # rows behind the stop row are not part of the flight
    got = _np(out['audit'])
    assert (got['status'] == 0).all()
    _compare(got, Xn, 4, 0.05 * rec_stride, 'gvf', rows=rows, t_start=2.0, d_safe=12.0, static=np.tile(np.array([disc]), (2, 1, 1)))


def test_tracking_history(ctx, gold):
    """A 2-aircraft tracking run of 50 rows through implement_controller_batch(audit=...)."""
    import full_sim as fs
    g = gold('tracking_trace_carestandin')
    T = 50
    time, xr, yr = g['time'][:T], g['x_ref'][:T, :2], g['y_ref'][:T, :2]
    out = fs.implement_controller_batch(time, xr, yr, (0.5, -0.3), g['X'][0][:2], audit=dict(n_ac=2, d_safe=8.0, err_tol=0.3))
    ctx.sync()
    X = out['X'].cpu().numpy()
    assert X.shape == (T, 5, 2)
    kw = dict(t_start=float(time[0]), x_ref=np.ascontiguousarray(xr), y_ref=np.ascontiguousarray(yr), d_safe=8.0, err_tol=0.3)
    _compare(_np(out['audit']), X, 2, float(time[1] - time[0]), 'tracking', check_margins=False, **kw)


def test_the_chain(ctx):
    """full_sim_phases_batch(audit=True) for one formation in a steady field around one moving disc: the three audits equal the CPU
    statement on the downloaded plan and histories; audit=None is the call without the argument, bit for bit."""
    import torch
    import d2d.multiopty_utils as d2mou
    import full_sim as fs
    import multi_opt_planner as mop
    import nlp_groups_wind_ref as G
    import wind_ref as WR
    from d2d.opty_utils import MovingObstacle

    class scen(mop.trap_4):
        cost = d2mou.CostComposit(kvel=70., kbank=1., kobs=10., kcol=10., vsp=12., obss=[], obs_kind=1, rcol=10)
    n_ac, c, X1_f, X2_f, X0B, ref3 = G.mission_inputs()
    F = WR.spline_of(lambda t, x, y: (1.0 + 0.0 * x, 0.0 * x))
    r, v, t_opt = 60, 15, 6
    ph1 = fs.CircularFormationGVF_batch(c[None], r, v, n_ac, X0f=X1_f[None, :, :3], X0=X0B[:1], record=(), windfield=F)
    ctx.sync()
    stop = ph1['stop_row'].cpu().numpy()
    t2 = float((min(stop[0], len(ph1['time'])) - 1) * 0.05)
    disc = [MovingObstacle((t2 - 37.0, t2 + 43.0), ((50.0, 40.0 - 400.0), (50.0, 40.0 + 400.0)), 8.0)]
    t_end = G.mission_t_end(stop, len(ph1['time']), 0.05, t_opt, ref3[0], 1)
    args = (c[None], r, v, n_ac, X1_f, scen, X2_f, t_opt)
    kw = dict(ref3=ref3, t_sim_end=t_end, X0=X0B[:1], windfield=F, moving_obstacles=disc, record3=('X',))
    out = fs.full_sim_phases_batch(*args, audit=True, **kw)
    ctx.sync()
    knots, dsc = (t.cpu().numpy() for t in out['plan']['moving'])
    t2d = out['plan']['t_start'].cpu().numpy()
    assert t2d[0] == t2 and len(out['phase3']) == 1 == len(out['audit']['phase3'])
    N2 = out['plan']['Xs'].shape[2]; dt2 = t_opt / (N2 - 1)
    Xs = out['plan']['Xs'].cpu().numpy()
    plan_hist = np.ascontiguousarray(Xs.transpose(2, 1, 0))
    base = dict(knots=knots, disc=dsc)
    for name, got, X, dt, kw_ref in (
            ('plan', out['audit']['plan'], plan_hist, dt2, dict(t_start=t2d)),
            ('phase2', out['audit']['phase2'], out['phase2']['X'].cpu().numpy(), dt2,
             dict(t_start=t2d, x_ref=np.ascontiguousarray(Xs[:, 0, :].T), y_ref=np.ascontiguousarray(Xs[:, 1, :].T))),
            ('phase3', out['audit']['phase3'][0], out['phase3'][0]['X'].cpu().numpy(), float(ref3[0][1] - ref3[0][0]),
             dict(t_start=t2d + t_opt, x_ref=np.ascontiguousarray(ref3[1]), y_ref=np.ascontiguousarray(ref3[2])))):
        got = _np(got)
        assert (got['status'] == 0).all(), name
        _compare(got, X, n_ac, dt, name, check_margins=False, **base, **kw_ref)
        print(name, 'separation', got['sep_dist'].min(), 'moving clearance', got['mov_clear'].min(), 'error', got.get('err_max', np.zeros(1)).max())
    a = fs.full_sim_phases_batch(*args, audit=None, **kw)
    b = fs.full_sim_phases_batch(*args, **kw)
    ctx.sync()
    assert 'audit' not in a and 'audit' not in b
    for x, y in ((a['plan']['Xs'], b['plan']['Xs']), (a['phase2']['X'], b['phase2']['X']), (a['phase3'][0]['X'], b['phase3'][0]['X']),
                 (a['plan']['Xs'], out['plan']['Xs']), (a['phase2']['X'], out['phase2']['X']), (a['phase3'][0]['X'], out['phase3'][0]['X'])):
        assert torch.equal(x, y)
