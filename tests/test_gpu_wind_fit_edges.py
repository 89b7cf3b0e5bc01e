"""GPU: d2d_wind_fit at the edges of its geometry -- short and straddling quads of drones, grids beyond one pass of the CG workgroup
up to D2D_WINDFIT_MAX_CP, a prior that meets data, the CG's terminal states, samples exactly on the box and on w_max, and the memory
contract of the C entry.  Nearly every assertion is a bit comparison against tests/wind_fit_ref.py (replay); tests/test_wind_fit_cpu.py
proves on the CPU that each input built there is what it claims to be."""
import ctypes as C

import numpy as np
import pytest

import wind_fit_ref as WF

pytestmark = pytest.mark.gpu

DT, W_MAX, LAM, MU, CG_TOL, CG_MAX = WF.EDGE_DT, WF.EDGE_W_MAX, WF.EDGE_LAM, WF.EDGE_MU, WF.EDGE_CG_TOL, WF.EDGE_CG_MAX
SMALL = {'steady-5x6': WF.edge_grid(1, 5, 6), 'unsteady-4x5x6': WF.edge_grid(4, 5, 6)}
FULL_ROWS, FULL_T_START = [130, 65, 2], [0.0, 3.0, 7.5]           # the (3, 4) history of the prior, cap and memory cases


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def _grid_c(g, cp=None):
    import d2dhip
    return d2dhip.WindFieldC(g.nt, g.ny, g.nx, 0, g.t0, g.ht, g.x0, g.hx, g.y0, g.hy, cp)


def _fit(ctx, X, n_ac, g, rows=None, t_start=None, prior=None, outputs=('support', 'stats', 'H', 'b'), dt=DT, **kw):
    import torch
    dX = ctx.dev(X)
    dr = None if rows is None else ctx.dev(np.asarray(rows, dtype=np.int32), dtype=torch.int32)
    dt0 = None if t_start is None else ctx.dev(np.asarray(t_start, dtype=np.float64))
    dp = None if prior is None else ctx.dev(np.ascontiguousarray(prior))
    args = dict(w_max=W_MAX, lam=LAM, mu=MU, cg_tol=CG_TOL, cg_max=CG_MAX)
    args.update(kw)
    out = ctx.wind_fit(dX, n_ac, dt, _grid_c(g), rows=dr, t_start=dt0, prior=dp, outputs=outputs, **args)
    ctx.sync()
    return {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in out.items()}


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _same(a, b, keys=('cp', 'support', 'H', 'b', 'stats')):
    return [k for k in keys if not _bits(a[k], b[k])]


def _planes(cp):
    """cp [nt][2][ny][nx] -> c [2][ncp] in the order of the unknowns."""
    return cp.transpose(1, 0, 2, 3).reshape(2, -1)


def _assert_replay(got, ref):
    """H, b, support and the counts of a fit are those of the CPU statement, bit for bit."""
    assert list(got['stats'][:4]) == [float(c) for c in ref['ms']['counts']]
    assert _bits(got['H'], ref['H'])
    assert _bits(got['b'], ref['b'])
    assert _bits(got['support'], ref['H'][:, ref['H'].shape[1] // 2])


def _assert_system(got, ref, g, lam=LAM, mu=MU, prior=None, label=''):
    """test_gpu_wind_fit.py's two derived bounds: H and b against plain fp64 A^T A and A^T m within the quantisation (2^-33 per sample
    and entry, times W for b, plus the fp64 reference's own summation error S^2 2^-53), and the residual of the REFERENCE system at
    the kernel's control points within 4 (cg_tol |rhs| + |dH|_F |c| + |db|)."""
    A, m = ref['A'], ref['m']
    S = ref['ms']['counts'][0]
    W = WF.w_pow2(W_MAX)
    qH = S * 2.0 ** -33 + S * S * 2.0 ** -53
    qb = qH * W
    H = (A.T @ A).tocsr()
    b = np.stack([A.T @ m[0], A.T @ m[1]])
    dH, db = np.abs(got['H'] - WF.stencil_of(H, g)).max(), np.abs(got['b'] - b).max()
    print(f'{label}: S = {S}, |dH| = {dH:.3e} (bound {qH:.3e}), |db| = {db:.3e} (bound {qb:.3e})')
    assert dH <= qH and db <= qb
    M, rhs = WF.system(H, b, g, lam, mu, prior=prior)
    ncp = g.nt * g.ny * g.nx
    c = _planes(got['cp'])
    for k in range(2):
        if not rhs[k].any():
            continue                                                 # (a zero right-hand side has its own assertions)
        res = np.linalg.norm(M @ c[k] - rhs[k])
        bound = 4.0 * (CG_TOL * np.linalg.norm(rhs[k]) + qH * np.sqrt(got['H'].size) * np.linalg.norm(c[k]) + qb * np.sqrt(ncp))
        print(f'  component {k}: |M c - rhs| = {res:.3e} (bound {bound:.3e}), {int(got["stats"][6])} CG iterations')
        assert res <= bound
    return A, m, c


# ---- 1. aircraft counts and short quads ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shape_refs():
    """Per (shape, grid): the history, the measurements, A and the replayed sums, computed once."""
    out = {}
    for shape, (rows, t_start) in WF.EDGE_SHAPES.items():
        X = WF.edge_history(*shape)
        for name, g in SMALL.items():
            ms = WF.measure(X, shape[1], DT, g, rows, t_start, W_MAX)
            A, m = WF.design(ms, g)
            H, b = WF.replay_blocks(ms, g, W_MAX)
            out[shape, name] = dict(X=X, rows=rows, t_start=t_start, ms=ms, A=A, m=m, H=H, b=b)
    return out


@pytest.mark.parametrize('name', list(SMALL))
@pytest.mark.parametrize('shape', list(WF.EDGE_SHAPES), ids=lambda s: '%dx%d' % s)
def test_every_quad_shape_is_the_replay_bit_for_bit(ctx, shape_refs, shape, name):
    """N = 9, 10, 1 and 64 drones: the last quad of a workgroup short by three, two, (three) and none, quads that straddle formations
    with their own rows and t_start, rows of exactly one unit (+ 0, 1, 2 samples).  H, b, support and the counts are the replay's; the
    residual sums are the fp64 ones at the kernel's control points."""
    g, ref = SMALL[name], shape_refs[shape, name]
    got = _fit(ctx, ref['X'], shape[1], g, ref['rows'], ref['t_start'])
    _assert_replay(got, ref)
    assert got['stats'][6] < CG_MAX and got['stats'][7] <= CG_TOL
    c = _planes(got['cp'])
    S = ref['ms']['counts'][0]
    rss = [float(np.sum((ref['A'] @ c[k] - ref['m'][k]) ** 2)) for k in range(2)]
    print(f'{shape} {name}: counts {ref["ms"]["counts"]}, rss {got["stats"][4:6]} against {rss}')
    assert np.allclose(got['stats'][4:6], rss, rtol=1e-9, atol=1e-12 * S)


@pytest.mark.parametrize('name', list(SMALL))
def test_nine_drones_do_not_depend_on_the_order_of_the_work(ctx, shape_refs, name):
    """(3, 3): bit-identical outputs for 1, 3, 7 wavefronts and the library's choice, and with the formations permuted."""
    g, ref = SMALL[name], shape_refs[(3, 3), name]
    X, rows, t_start = ref['X'], np.array(ref['rows']), np.array(ref['t_start'])
    base = _fit(ctx, X, 3, g, rows, t_start)
    _assert_replay(base, ref)
    perm = [2, 0, 1]
    Xp = np.ascontiguousarray(X.reshape(WF.EDGE_ROWS, 5, 3, 3)[:, :, perm].reshape(WF.EDGE_ROWS, 5, -1))
    others = [_fit(ctx, X, 3, g, rows, t_start, waves=w) for w in (0, 1, 3, 7)] + [_fit(ctx, Xp, 3, g, rows[perm], t_start[perm])]
    for o in others:
        assert not _same(o, base, ('cp', 'support', 'H', 'b'))
        assert list(o['stats'][:4]) == list(base['stats'][:4]) and list(o['stats'][6:]) == list(base['stats'][6:])


@pytest.mark.parametrize('name', list(SMALL))
def test_negative_rows_are_zero_rows(ctx, shape_refs, name):
    g, ref = SMALL[name], shape_refs[(3, 3), name]
    a = _fit(ctx, ref['X'], 3, g, [130, -5, 2], ref['t_start'])
    b = _fit(ctx, ref['X'], 3, g, [130, 0, 2], ref['t_start'])
    assert not _same(a, b)
    assert a['stats'][0] < ref['ms']['counts'][0]                    # (the formation that left did hold samples)


# ---- 2. grid sizes across the CG workgroup -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big_history():
    B = WF.EDGE_BIG
    return WF.edge_history(*B['shape'], corners=B['corners'])


@pytest.mark.parametrize('name', list(WF.EDGE_BIG_GRIDS))
def test_grids_beyond_one_pass_of_the_cg_workgroup(ctx, big_history, name):
    """667, 715 and twice 4096 control points (D2D_WINDFIT_MAX_CP exactly): the strided loops of the CG workgroup run more than once,
    the row tail meets a count that is no multiple of 4, the staged iterate fills its LDS array.  The history holds samples in the
    first and the last cell (tests/test_wind_fit_cpu.py), so the largest indices and the -1 partners are used."""
    B, g = WF.EDGE_BIG, WF.edge_grid(*WF.EDGE_BIG_GRIDS[name])
    ms = WF.measure(big_history, B['shape'][1], DT, g, B['rows'], B['t_start'], W_MAX)
    A, m = WF.design(ms, g)
    Hs, bs, _, _ = WF.replay(ms, g, W_MAX)
    ref = dict(ms=ms, A=A, m=m, H=Hs, b=bs)
    got = _fit(ctx, big_history, B['shape'][1], g, B['rows'], B['t_start'])
    _assert_replay(got, ref)
    print(f'{name}: {int(got["stats"][6])} CG iterations, residual {got["stats"][7]:.3e}')
    assert got['stats'][6] < CG_MAX and got['stats'][7] <= CG_TOL
    _, _, c = _assert_system(got, ref, g, label=name)
    S = ms['counts'][0]
    rss = [float(np.sum((A @ c[k] - m[k]) ** 2)) for k in range(2)]
    assert np.allclose(got['stats'][4:6], rss, rtol=1e-9, atol=1e-12 * S)


# ---- 3. a prior that meets data ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def full():
    """The (3, 4) history with its usual rows on the two small grids."""
    X = WF.edge_history(3, 4)
    out = dict(X=X)
    for name, g in SMALL.items():
        ms = WF.measure(X, 4, DT, g, FULL_ROWS, FULL_T_START, W_MAX)
        A, m = WF.design(ms, g)
        Hs, bs, _, _ = WF.replay(ms, g, W_MAX)
        out[name] = dict(ms=ms, A=A, m=m, H=Hs, b=bs)
    return out


@pytest.mark.parametrize('mu', [MU, 1e-2])
@pytest.mark.parametrize('name', list(SMALL))
def test_prior_with_data_meets_the_reference_system(ctx, full, name, mu):
    """A prior that differs in every entry, with the full history: rhs = b + mu c_prior and the start c = c_prior in wf_prior's
    [nt][2][ny][nx] layout.  At the usual mu = 1e-4, and at mu = 1e-2, where a misplaced prior moves the right-hand side (by mu times
    the difference of two entries, 0.09 at the least) far above the bound."""
    g, ref = SMALL[name], full[name]
    prior = WF.edge_prior(g)
    assert len(np.unique(prior)) == prior.size
    got = _fit(ctx, full['X'], 4, g, FULL_ROWS, FULL_T_START, prior=prior, mu=mu)
    _assert_replay(got, ref)
    assert got['stats'][6] < CG_MAX and got['stats'][7] <= CG_TOL
    _assert_system(got, ref, g, mu=mu, prior=prior, label=name)


@pytest.mark.parametrize('name', list(SMALL))
def test_without_smoothing_an_unbacked_control_point_is_the_prior(ctx, full, name):
    """lam = 0: a control point whose row of H is zero is coupled to nothing, and cp there is the prior bit for bit.  Steady, these are
    all points with support == 0.  Unsteady, the fixed point leaves points whose support (a sum of squares of weights below 2^-16.5,
    each rounded to 0) is 0 while products with larger weights are not: include/d2d.h states that support == 0 does not make the row
    zero, and the exact statement is made for zero rows."""
    g, ref = SMALL[name], full[name]
    prior = WF.edge_prior(g)
    got = _fit(ctx, full['X'], 4, g, FULL_ROWS, FULL_T_START, prior=prior, lam=0.0)
    _assert_replay(got, ref)
    alone = ~got['H'].any(axis=1)
    assert alone.any() and not alone.all()
    assert not (got['support'][alone] != 0).any()
    if name == 'steady-5x6':
        assert np.array_equal(alone, got['support'] == 0)
    assert _bits(_planes(got['cp'])[:, alone], _planes(prior)[:, alone])
    assert np.isfinite(got['cp']).all() and (_planes(got['cp'])[:, ~alone] != _planes(prior)[:, ~alone]).any()


@pytest.mark.parametrize('name', list(SMALL))
def test_components_do_not_see_each_other(ctx, full, name):
    """Two priors that differ in the y planes only: the x planes of cp are the same bits (one component freezes while the other still
    iterates), the y planes differ."""
    g = SMALL[name]
    a = _fit(ctx, full['X'], 4, g, FULL_ROWS, FULL_T_START, prior=WF.edge_prior(g), mu=1e-2)
    b = _fit(ctx, full['X'], 4, g, FULL_ROWS, FULL_T_START, prior=WF.edge_prior(g, y_shift=-25.0), mu=1e-2)
    assert _bits(a['cp'][:, 0], b['cp'][:, 0])
    assert (a['cp'][:, 1] != b['cp'][:, 1]).any()
    assert a['stats'][7] <= CG_TOL and b['stats'][7] <= CG_TOL


# ---- 4. the CG's terminal states -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cg_max', [1, 3])
def test_iteration_cap_returns_that_iterate(ctx, full, cg_max):
    """cg_max reached before cg_tol: stats[6] == cg_max, stats[7] > cg_tol and stats[7] is the TRUE relative residual of the returned
    cp in the system of the kernel's own H and b (rtol 1e-6: the recursive residual drifts from the true one by about iterations x
    eps x cond(M), below 1e-9 here).  cp is iterate cg_max of wind_fit_ref.pcg.  The tolerance is measured, not chosen: the distance
    between pcg in fp64 and in long double at that iterate is how far a valid fp64 evaluation lies from the exact iterate; the kernel
    (butterfly sums, fma) is allowed 8 times that from the long-double iterate.  Measured on an MI355X (component x, y):
    cg_max = 1: gap 1.13e-15, 2.30e-15, kernel 1.36e-15, 2.05e-15; cg_max = 3: gap 1.34e-14, 5.03e-15, kernel 2.36e-14, 2.46e-15
    (control points of magnitude 4 to 6: the gaps are 2 to 30 units in the last place)."""
    g, mu = SMALL['steady-5x6'], 1e-2
    got = _fit(ctx, full['X'], 4, g, FULL_ROWS, FULL_T_START, mu=mu, cg_max=cg_max)
    _assert_replay(got, full['steady-5x6'])
    assert got['stats'][6] == cg_max and got['stats'][7] > CG_TOL
    assert np.isfinite(got['cp']).all()
    M, rhs = WF.system(WF.matrix_of(got['H'], g), got['b'], g, LAM, mu)
    c = _planes(got['cp'])
    true = max(np.linalg.norm(M @ c[k] - rhs[k]) / np.linalg.norm(rhs[k]) for k in range(2))
    print(f'cg_max = {cg_max}: reported residual {got["stats"][7]:.9e}, true {true:.9e}')
    assert abs(got['stats'][7] - true) <= 1e-6 * true
    for k in range(2):
        x64 = WF.pcg(M, rhs[k], np.zeros(c.shape[1]), cg_max, tol=CG_TOL)
        xld = WF.pcg(M, rhs[k], np.zeros(c.shape[1]), cg_max, tol=CG_TOL, longdouble=True)
        gap = float(np.abs(x64 - xld).max())
        err = float(np.abs(c[k] - xld).max())
        print(f'  component {k}: |pcg64 - pcg80| = {gap:.3e}, |kernel - pcg80| = {err:.3e} (allowed {8.0 * gap:.3e}), |x| = {np.abs(x64).max():.3e}')
        assert gap > 0.0 and err <= 8.0 * gap


def test_zero_right_hand_side_is_frozen_at_zero(ctx):
    """psi = 0 and constant y: every m_y is exactly 0, so b[1] is, and with no prior the y system has a zero right-hand side.  The
    header: that component is frozen at its start, c = 0, and contributes 0 to the reported residual; the x component is solved."""
    g = SMALL['steady-5x6']
    X = WF.zero_rhs_history()
    ms = WF.measure(X, 4, DT, g, None, None, W_MAX)
    A, m = WF.design(ms, g)
    Hs, bs, _, _ = WF.replay(ms, g, W_MAX)
    ref = dict(ms=ms, A=A, m=m, H=Hs, b=bs)
    got = _fit(ctx, X, 4, g)
    _assert_replay(got, ref)
    assert not got['b'][1].any() and got['b'][0].any()
    assert not got['cp'][:, 1].any()
    assert got['stats'][5] == 0.0 and got['stats'][4] > 0.0
    assert np.isfinite(got['stats'][7]) and got['stats'][7] <= CG_TOL and 0 < got['stats'][6] < CG_MAX
    _assert_system(got, ref, g, label='zero rhs')


# ---- 5. samples on the edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('origin', [False, True], ids=['box', 'minus-zero'])
@pytest.mark.parametrize('w_max', list(WF.SAMPLE_EDGE_COUNTS))
def test_samples_on_the_box_and_on_w_max(ctx, w_max, origin):
    """The hand-built history of wind_fit_ref.sample_edge_case: midpoints exactly on the upper and the lower corner of the box (inside;
    origin: the lower one through s = -0.0), |m_x| = w_max exactly (accepted) and 2^-36 above (rejected), w_max a power of two (m / W
    = 1, the largest fixed-point value) and just above one (W doubles), psi = -1e6, 1e6, -0.0.  Counts stated by hand."""
    X, g = WF.sample_edge_case(origin)
    ms = WF.measure(X, 1, WF.SAMPLE_EDGE_DT, g, WF.SAMPLE_EDGE_ROWS, None, w_max)
    Hs, bs, _, _ = WF.replay(ms, g, w_max)
    got = _fit(ctx, X, 1, g, WF.SAMPLE_EDGE_ROWS, None, dt=WF.SAMPLE_EDGE_DT, w_max=w_max)
    assert list(got['stats'][:4]) == [float(c) for c in WF.SAMPLE_EDGE_COUNTS[w_max]]
    _assert_replay(got, dict(ms=ms, H=Hs, b=bs))
    assert got['support'][-1] > 0 and got['support'][0] > 0          # the two corner control points are backed: the edge is inside
    assert got['stats'][7] <= CG_TOL and np.isfinite(got['cp']).all()


# ---- 6. the memory contract of the C entry -------------------------------------------------------------------------------------------
GUARD = 4096


class _Raw:
    """d2d_wind_fit through ctypes with every device buffer between two guards of GUARD bytes of 0xA5."""

    def __init__(self, ctx, X, n_ac, g, rows, t_start, mu=MU, cg_max=CG_MAX):
        import d2dhip
        import torch
        self.ctx, self.torch, self.g = ctx, torch, g
        n_rows, _, N = X.shape
        self.p = d2dhip.WindFitParams(N // n_ac, n_ac, n_rows, cg_max, 0, 0, DT, W_MAX, LAM[0], LAM[1], LAM[2], mu, CG_TOL)
        self.gc = _grid_c(g)
        self.X = ctx.dev(X)
        self.rows = ctx.dev(np.asarray(rows, dtype=np.int32), dtype=torch.int32)
        self.t_start = ctx.dev(np.asarray(t_start, dtype=np.float64))
        self.nwork = int(ctx.lib.d2d_wind_fit_workspace(C.byref(self.p), C.byref(self.gc)))
        assert self.nwork > 0 and self.nwork % 16 == 0
        ncp = g.nt * g.ny * g.nx
        self.sizes = dict(cp=2 * ncp * 8, support=ncp * 8, stats=8 * 8, H=ncp * (49 if g.nt == 1 else 343) * 8, b=2 * ncp * 8, work=self.nwork)

    def buffers(self):
        return {k: self.torch.full((n + 2 * GUARD,), 0xA5, dtype=self.torch.uint8, device=self.ctx.device) for k, n in self.sizes.items()}

    def run(self, bufs, want=('support', 'stats', 'H', 'b'), null_out=False):
        import d2dhip
        for k, n in self.sizes.items():
            if k != 'work':
                bufs[k][GUARD:GUARD + n] = 0x5A                      # (payloads start from junk; the guards keep 0xA5)
        ptr = lambda k: C.c_void_p(bufs[k].data_ptr() + GUARD)       # noqa: E731
        o = d2dhip.WindFitOut(*[ptr(k) if k in want else None for k in ('support', 'stats', 'H', 'b')])
        rc = self.ctx.lib.d2d_wind_fit(self.ctx.h, C.byref(self.p), C.c_void_p(self.X.data_ptr()), C.c_void_p(self.rows.data_ptr()),
                                       C.c_void_p(self.t_start.data_ptr()), C.byref(self.gc), ptr('cp'), ptr('work'),
                                       None if null_out else C.byref(o))
        assert rc == 0
        self.ctx.sync()
        out = {k: bufs[k][GUARD:GUARD + n].cpu().numpy().view(np.float64) for k, n in self.sizes.items() if k != 'work'}
        guards = {k: bool((bufs[k][:GUARD] == 0xA5).all().item() and (bufs[k][GUARD + n:] == 0xA5).all().item()) for k, n in self.sizes.items()}
        return out, guards


@pytest.mark.parametrize('name', list(SMALL))
def test_result_does_not_depend_on_what_the_workspace_held(ctx, full, name):
    """"work: overwritten": 0xFF bytes (NaNs as doubles, -1 as integers), zeros, and what a fit on the other grid left behind give the
    same bits on every output, and they are the replay's."""
    g = SMALL[name]
    raw = _Raw(ctx, full['X'], 4, g, FULL_ROWS, FULL_T_START)
    other = _Raw(ctx, full['X'], 4, [v for k, v in SMALL.items() if k != name][0], FULL_ROWS, FULL_T_START)
    results = []
    for fill in (0xFF, 0x00, 'other'):
        bufs = raw.buffers()
        if fill == 'other':
            ob = other.buffers()
            other.run(ob)
            n = min(other.nwork, raw.nwork)
            bufs['work'][GUARD:GUARD + n] = ob['work'][GUARD:GUARD + n]
        else:
            bufs['work'][GUARD:GUARD + raw.nwork] = fill
        out, guards = raw.run(bufs)
        assert all(guards.values()), guards
        results.append(out)
    for o in results[1:]:
        assert not _same(o, results[0])
    ref = full[name]
    assert _bits(results[0]['H'].reshape(ref['H'].shape), ref['H']) and _bits(results[0]['b'].reshape(ref['b'].shape), ref['b'])
    assert list(results[0]['stats'][:4]) == [float(c) for c in ref['ms']['counts']]


@pytest.mark.parametrize('name', ['steady-5x6', 'steady-64x64', 'unsteady-4x32x32'])
def test_no_kernel_writes_outside_the_advertised_sizes(ctx, big_history, name):
    """Guards of 4 KiB in front of and behind the workspace of d2d_wind_fit_workspace() bytes, cp_out, support, stats, H_out and b_out
    are untouched, at the smallest grid and at both grids of D2D_WINDFIT_MAX_CP control points."""
    B = WF.EDGE_BIG
    g = SMALL[name] if name in SMALL else WF.edge_grid(*WF.EDGE_BIG_GRIDS[name])
    raw = _Raw(ctx, big_history, B['shape'][1], g, B['rows'], B['t_start'])
    out, guards = raw.run(raw.buffers())
    assert all(guards.values()), guards
    ms = WF.measure(big_history, B['shape'][1], DT, g, B['rows'], B['t_start'], W_MAX)
    assert list(out['stats'][:4]) == [float(c) for c in ms['counts']]
    assert np.isfinite(out['cp']).all() and out['stats'][7] <= CG_TOL
    assert not (out['support'].view(np.uint64) == 0x5A5A5A5A5A5A5A5A).any() and not (out['cp'].view(np.uint64) == 0x5A5A5A5A5A5A5A5A).any()


@pytest.mark.parametrize('name', list(SMALL))
def test_every_selection_of_outputs_gives_the_same_bits(ctx, full, name):
    """d2d_windfit_out "any NULL", and out == NULL: cp and the member asked for are those of the call with every output, an output
    not asked for is not written, and cp does not need the residual pass (stats NULL)."""
    raw = _Raw(ctx, full['X'], 4, SMALL[name], FULL_ROWS, FULL_T_START)
    base, guards = raw.run(raw.buffers())
    assert all(guards.values())
    for want in ((), ('support',), ('stats',), ('H',), ('b',)):
        for null_out in ((True, False) if not want else (False,)):
            out, guards = raw.run(raw.buffers(), want=want, null_out=null_out)
            assert all(guards.values()), (want, guards)
            assert not _same(out, base, ('cp',) + want), (want, null_out)
            for k in set(('support', 'stats', 'H', 'b')) - set(want):
                assert (out[k].view(np.uint64) == 0x5A5A5A5A5A5A5A5A).all(), (want, k)
