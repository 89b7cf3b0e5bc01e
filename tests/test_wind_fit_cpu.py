"""CPU: the wind-field estimator as tests/wind_fit_ref.py states it (include/d2d.h d2d_wind_fit), the host classes around it and
the ABI's declarations.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import wind_fit_ref as WF
import wind_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECOVERY_ERR = WF.RECOVERY_ERR      # what test_recovery_of_truth measured: the baseline of the GPU recovery test, which allows twice as much


@pytest.fixture(scope='module')
def flights():
    out = {}
    for name in ('shear', 'gust'):
        F, grid, _, lam = WF.recovery_case(name)
        X, _, _ = R.formation_gvf_run_wind(WF.RECOVERY_C, WF.RECOVERY_R, WF.RECOVERY_V, WF.recovery_x0(), WF.RECOVERY_STEPS,
                                           WF.RECOVERY_DT, F)
        out[name] = (F, grid, lam, X)
    return out


@pytest.mark.parametrize('name', ['shear', 'gust'])
def test_recovery_of_truth(flights, name):
    """A formation flown by the CPU plant (wind_ref.formation_gvf_run_wind, 120 rows of 0.05 s) in wind_ref.shear (steady) and
    wind_ref.gust (unsteady), fitted on a 40 m (x 2 s) grid over the flown region.  Measured here, largest |F^ - F| at the flown
    midpoints: shear 6.41e-3 m/s, gust 3.23e-2 m/s (wind_fit_ref.RECOVERY_ERR rounds them up), beside the largest error of a single measurement,
    0.100 m/s in both -- the first row, where the bank angle jumps within one step and psi'' is large; the smooth-flight
    trapezoid estimate dt^2 / 12 v psidot^2 is 1.8e-2 m/s.  The fit averages the measurements: it must not be worse than the worst
    of them, and it stays within the recorded value."""
    F, grid, lam, X = flights[name]
    Xh = np.ascontiguousarray(X.transpose(0, 2, 1))
    out = WF.fit(Xh, 4, WF.RECOVERY_DT, grid, lam=lam, mu=1e-6)
    assert out['stats'][0] == (WF.RECOVERY_STEPS - 1) * 4 and out['stats'][1:4].sum() == 0
    err, meas = WF.recovery_error(out['cp'], grid, F, out['ms'])
    psid = np.abs(np.diff(np.unwrap(X[:, :, 2], axis=0), axis=0)).max() / WF.RECOVERY_DT
    trap = WF.RECOVERY_DT ** 2 / 12 * X[:, :, 4].max() * psid ** 2
    print(f'{name}: max|F^ - F| = {err:.3e}, max|m - F| = {meas:.3e}, dt^2/12 v psidot^2 = {trap:.3e}')
    assert err <= meas
    assert err <= RECOVERY_ERR[name]


def _straight(w, headings, n_rows=40, dt=0.05, v=12.0, p0=(0.0, 0.0)):
    """Straight constant-speed flights in the constant wind w: X [n_rows][5][len(headings)]."""
    t = np.arange(n_rows) * dt
    X = np.zeros((n_rows, 5, len(headings)))
    for d, psi in enumerate(headings):
        X[:, 0, d] = p0[0] + 3.0 * d + (v * np.cos(psi) + w[0]) * t
        X[:, 1, d] = p0[1] - 2.0 * d + (v * np.sin(psi) + w[1]) * t
        X[:, 2, d], X[:, 4, d] = psi, v
    return X


def test_exact_case_constant_wind():
    """Straight flight at constant speed in a constant wind: the trapezoid rule is exact, so with a smoothness weight the constant is
    found in every control point the data backs (and, the penalty having constants in its null space, in the others too); without one
    (lam = 0) a control point without support is exactly the prior while the field along the flown paths is still the constant."""
    w = (3.0, -1.5)
    X = _straight(w, [0.3, 1.9, -2.4, 4.0])
    grid = WF.grid_over(np.arange(-40.0, 41.0, 20.0), np.arange(-40.0, 41.0, 20.0))
    out = WF.fit(X, 4, 0.05, grid, lam=1.0, mu=1e-14)        # (the pull towards the prior 0 biases c by mu |w| / lambda_min: negligible here)
    assert out['stats'][0] == 39 * 4
    sup = out['support'] > 0
    assert sup.any() and not sup.all()
    assert np.abs(out['c'][0][sup] - w[0]).max() <= 1e-10 and np.abs(out['c'][1][sup] - w[1]).max() <= 1e-10
    prior = (7.0, -3.0)
    out = WF.fit(X, 4, 0.05, grid, lam=0.0, mu=1e-9, prior=prior)
    sup = out['support'] > 0
    assert np.array_equal(out['c'][0][~sup], np.full((~sup).sum(), prior[0])) and np.array_equal(out['c'][1][~sup], np.full((~sup).sum(), prior[1]))
    res = np.stack([out['A'] @ out['c'][k] - w[k] for k in range(2)])
    # the pull towards the prior leaves, in a direction of H with eigenvalue l, the data residual sqrt(l) mu / (l + mu) |prior - w|
    # <= sqrt(mu) / 2 |prior - w|: the bound on the residual's 2-norm, and so on its largest entry
    delta = np.sqrt(out['c'].shape[1] * ((prior[0] - w[0]) ** 2 + (prior[1] - w[1]) ** 2))
    assert np.abs(res).max() <= 0.5 * np.sqrt(1e-9) * delta


def test_rejections_are_counted_and_do_not_leak():
    """A NaN row, a flight that leaves the box and a jump above w_max: each is counted under its reason, and H, b are those of the
    history with the offending samples removed."""
    w = (1.0, 0.5)
    grid = WF.grid_over(np.arange(-40.0, 41.0, 20.0), np.arange(-40.0, 41.0, 20.0))
    X = _straight(w, [0.3, 1.9, -2.4, 0.0], n_rows=60)
    X[:, 0, 3] += 20.0                                   # drone 3 flies +x from x = 29: it leaves the box (x <= 40) on the way
    X[10, 3, 0] = np.nan                                 # phi is never used, but a broken row is a broken row: samples 9 and 10 of drone 0
    X[20:, 1, 1] += 5.0                                  # a 5 m jump in one row of 0.05 s: 100 m/s, sample 19 of drone 1
    ms = WF.measure(X, 4, 0.05, grid, w_max=30.0)
    n_out = int(((ms['px'][:, 3] > 40.0)).sum())
    assert n_out > 0 and ms['counts'] == [59 * 4 - 3 - n_out, 2, n_out, 1]
    assert (ms['why'][[9, 10], 0] == 1).all() and ms['why'][19, 1] == 3 and (ms['why'][:, 2] == 0).all()
    A, m = WF.design(ms, grid)
    assert A.shape[0] == ms['counts'][0] and np.isfinite(A.data).all() and np.isfinite(m).all()
    # the same H from the samples one by one, the rejected ones left out by hand
    keep = np.ones((59, 4), bool); keep[[9, 10], 0] = False; keep[19, 1] = False; keep[ms['px'][:, 3] > 40.0, 3] = False
    assert np.array_equal(keep, ms['why'] == 0)
    # rows / t_start: a formation with fewer than two rows contributes nothing
    ms2 = WF.measure(X, 2, 0.05, grid, rows=[60, 1], w_max=30.0)
    assert (ms2['why'][:, 2:] == -1).all() and sum(ms2['counts']) == 59 * 2
    # the fixed-point replay is the plain fp64 A^T A within its documented quantisation: 2^-33 per sample and entry
    Hs, bs, _, _ = WF.replay(ms, grid, 30.0)
    H = WF.stencil_of(A.T @ A, grid)
    S = ms['counts'][0]
    assert np.abs(Hs - H).max() <= S * 2.0 ** -33 + S * 2.0 ** -52
    b = np.stack([A.T @ m[0], A.T @ m[1]])
    assert np.abs(bs - b).max() <= S * 2.0 ** -33 * 32.0 + S * 2.0 ** -52 * 32.0


def test_sincos_is_cos_and_sin():
    a = np.concatenate([np.linspace(-40.0, 40.0, 20001), [0.0, np.pi / 4, -np.pi / 4, 1e5, -1e6]])
    c, s = WF.sincos(a)
    assert np.abs(c - np.cos(a)).max() <= 4e-16 and np.abs(s - np.sin(a)).max() <= 4e-16


def test_estimator_validation_names_the_argument():
    from d2d.wind import SplineWindField, WindEstimator
    x, y = np.arange(0.0, 101.0, 20.0), np.arange(-50.0, 51.0, 25.0)
    e = WindEstimator(x, y, lam=(1e-2, 2e-2, 0.0), mu=1e-5, prior=(1.0, -2.0), rec_stride=4)
    g = e.geometry()
    assert (g['nt'], g['ny'], g['nx'], g['x0'], g['hx'], g['y0'], g['hy']) == (1, 7, 8, 0.0, 20.0, -50.0, 25.0)
    assert e.prior.shape == (1, 2, 7, 8) and e.rec_stride == 4 and e.lam == (1e-2, 2e-2, 0.0)
    assert WindEstimator(x, y, t=np.arange(0.0, 9.0, 2.0)).geometry()['nt'] == 7
    same = SplineWindField(np.zeros((1, 2, 7, 8)), 0.0, 20.0, -50.0, 25.0)
    assert WindEstimator(x, y, prior=same).prior.shape == (1, 2, 7, 8)
    for kw, word in ((dict(mu=0.0), 'mu'), (dict(mu=np.nan), 'mu'), (dict(lam=-1.0), 'lam'), (dict(lam=(1.0, 2.0)), 'lam'),
                     (dict(w_max=0.0), 'w_max'), (dict(rec_stride=0), 'rec_stride'), (dict(rec_stride=1.5), 'rec_stride'),
                     (dict(prior=(1.0, 2.0, 3.0)), 'prior'), (dict(prior=SplineWindField(np.zeros((1, 2, 7, 8)), 5.0, 20.0, -50.0, 25.0)), 'prior'),
                     (dict(cg_tol=1.0), 'cg_tol'), (dict(t=np.arange(0.0, 200.0, 1.0)), 'control points')):
        with pytest.raises(ValueError, match=word):
            WindEstimator(x, y, **kw)
    with pytest.raises(ValueError, match='x'):
        WindEstimator([0.0, 1.0, 3.0], y)


def test_header_binding_and_signatures():
    import d2dhip
    import full_sim
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 122
    assert re.search(r'\bint d2d_wind_fit\(', hdr) and re.search(r'\bint64_t d2d_wind_fit_workspace\(', hdr)
    for fn in ('d2d_wind_fit', 'd2d_wind_fit_workspace'):
        assert fn in d2dhip.EXPORTS
    plain = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for struct, cls in (('d2d_windfit_params', d2dhip.WindFitParams), ('d2d_windfit_out', d2dhip.WindFitOut)):
        body = re.search(r'typedef struct \{([^}]*)\} %s;' % struct, plain).group(1)
        names = [n.strip().lstrip('*') for decl in re.findall(r'(?:const )?(?:uint64_t|int64_t|int32_t|double) ([^;]+);', body) for n in decl.split(',')]
        assert names == [k for k, _ in cls._fields_], struct
    val = lambda name: int(re.search(r'#define %s (\d+)' % name, hdr).group(1))       # noqa: E731
    assert (d2dhip.WINDFIT_MAX_CP, d2dhip.WINDFIT_CHUNK) == (val('D2D_WINDFIT_MAX_CP'), val('D2D_WINDFIT_CHUNK')) == (4096, WF.CHUNK)
    assert len(d2dhip.WINDFIT_STATS) == 8
    for fn in (full_sim.full_sim_phases_batch, full_sim.CircularFormationGVF_batch, full_sim.implement_controller_batch):
        assert inspect.signature(fn).parameters['wind_estimate'].default is None
    p = inspect.signature(d2dhip.Context.wind_fit).parameters
    assert p['rows'].default is None and p['t_start'].default is None and p['prior'].default is None and p['outputs'].default is None
    with pytest.raises(TypeError, match='WindEstimator'):
        full_sim.CircularFormationGVF_batch(np.zeros((1, 4, 2)), 60, 15, 4, wind_estimate=object())
    from d2d.wind import WindEstimator
    with pytest.raises(ValueError, match="'X' must be in record"):
        full_sim.CircularFormationGVF_batch(np.zeros((1, 4, 2)), 60, 15, 4, record=(), wind_estimate=WindEstimator(np.arange(4.0), np.arange(4.0)))


# ---- the inputs of tests/test_gpu_wind_fit_edges.py: each is what it claims to be, by the reference alone ---------------------------
EDGE_SMALL = [(1, 5, 6), (4, 5, 6)]


@pytest.mark.parametrize('shape', list(WF.EDGE_SHAPES), ids=lambda s: '%dx%d' % s)
def test_edge_histories_hold_what_the_gpu_cases_need(shape):
    """Every (n_form, n_ac) of the quad cases: all samples of the stated rows are accounted for, most are used, every rejection
    occurs where there are three drones or more, the headings reach -1e5 and 1e5, and the blocked replay is the replay."""
    rows, t_start = WF.EDGE_SHAPES[shape]
    n_form, n_ac = shape
    X = WF.edge_history(n_form, n_ac)
    assert X.shape == (WF.EDGE_ROWS, 5, n_form * n_ac) and len(rows) == n_form and len(set(t_start)) == n_form
    assert max(rows) <= 130 and n_form * n_ac <= 64
    for gd in EDGE_SMALL:
        g = WF.edge_grid(*gd)
        ms = WF.measure(X, n_ac, WF.EDGE_DT, g, rows, t_start, WF.EDGE_W_MAX)
        assert sum(ms['counts']) == sum(r - 1 for r in rows) * n_ac
        assert ms['counts'][0] >= 0.75 * sum(ms['counts'])
        if n_form * n_ac >= 3:
            assert ms['counts'][1] == 2 and ms['counts'][2] > 0
        if shape in ((3, 3), (1, 64)):
            assert ms['counts'][3] == 1
            assert X[:, 2].min() < -9e4 and X[:, 2].max() > 9e4
        if gd[0] > 1:
            assert len(set(ms['seg'][0][ms['why'] == 0])) == 1       # nt = 4: one time cell, every t_start inside it
        if shape == (3, 3):
            Hs, bs, _, _ = WF.replay(ms, g, WF.EDGE_W_MAX)
            Hb, bb = WF.replay_blocks(ms, g, WF.EDGE_W_MAX, block=2)
            assert np.array_equal(Hs, Hb) and np.array_equal(bs, bb)
            assert np.array_equal(WF.stencil_of(WF.matrix_of(Hs, g), g), Hs)
            lost = WF.measure(X, n_ac, WF.EDGE_DT, g, [130, -5, 2], t_start, WF.EDGE_W_MAX)
            assert lost['counts'] == WF.measure(X, n_ac, WF.EDGE_DT, g, [130, 0, 2], t_start, WF.EDGE_W_MAX)['counts']
            assert lost['counts'][0] < ms['counts'][0]


@pytest.mark.parametrize('name', list(WF.EDGE_BIG_GRIDS))
def test_big_grid_history_reaches_the_first_and_the_last_cell(name):
    """667, 715, 4096 and 4096 control points; a few hundred samples; used samples in the cell of the first row AND column of cells
    (at the first time cell) and in the cell of the last row AND column (at the last time cell): the largest control-point index
    is backed, and the stencils there have partners outside the grid."""
    B, g = WF.EDGE_BIG, WF.edge_grid(*WF.EDGE_BIG_GRIDS[name])
    ncp = g.nt * g.ny * g.nx
    assert ncp == {'steady-23x29': 667, 'unsteady-5x11x13': 715}.get(name, 4096) and ncp <= 4096
    X = WF.edge_history(*B['shape'], corners=B['corners'])
    ms = WF.measure(X, B['shape'][1], WF.EDGE_DT, g, B['rows'], B['t_start'], WF.EDGE_W_MAX)
    assert 300 <= ms['counts'][0] <= 500 and max(B['rows']) <= 130
    use = ms['why'] == 0
    it, iy, ix = (s[use] for s in ms['seg'])
    t_last = g.nt - 4 if g.nt > 1 else 0
    assert ((it == 0) & (iy == 0) & (ix == 0)).any()
    assert ((it == t_last) & (iy == g.ny - 4) & (ix == g.nx - 4)).any()
    if g.nt > 4:
        assert t_last > 0 and (it == 0).any() and (it == t_last).any()
    Hs, _, _, _ = WF.replay(ms, g, WF.EDGE_W_MAX)
    sup = Hs[:, Hs.shape[1] // 2]
    assert sup[0] > 0 and sup[-1] > 0
    assert (WF.stencil_index(g)[-1] == -1).any()


@pytest.mark.parametrize('gd', EDGE_SMALL, ids=['steady-5x6', 'unsteady-4x5x6'])
def test_prior_case_leaves_control_points_unbacked(gd):
    """The (3, 4) history on the small grids: some control points have an all-zero row of the replayed H (and a zero b): without
    smoothing they are coupled to nothing.  Steady these are exactly the points with support == 0.  Unsteady the fixed point makes
    support == 0 the larger set (weights below 2^-16.5 square to 0, their products with larger weights do not): include/d2d.h says
    so, and the GPU test makes its exact statement for the zero rows.  The prior differs in every entry."""
    g = WF.edge_grid(*gd)
    X = WF.edge_history(3, 4)
    ms = WF.measure(X, 4, WF.EDGE_DT, g, [130, 65, 2], [0.0, 3.0, 7.5], WF.EDGE_W_MAX)
    Hs, bs, _, _ = WF.replay(ms, g, WF.EDGE_W_MAX)
    sup = Hs[:, Hs.shape[1] // 2]
    alone = ~Hs.any(axis=1)
    assert alone.any() and not alone.all() and not bs[:, alone].any() and not sup[alone].any()
    if g.nt == 1:
        assert np.array_equal(alone, sup == 0)
    else:
        assert (sup == 0).sum() > alone.sum()
    prior = WF.edge_prior(g)
    assert prior.shape == (g.nt, 2, g.ny, g.nx) and len(np.unique(prior)) == prior.size
    other = WF.edge_prior(g, y_shift=-25.0)
    assert np.array_equal(other[:, 0], prior[:, 0]) and (other[:, 1] != prior[:, 1]).all()
    # without smoothing the direct solve returns the prior there (to rounding: the GPU's CG returns it exactly)
    M, rhs = WF.system(WF.matrix_of(Hs, g), bs, g, 0.0, WF.EDGE_MU, prior=prior)
    pv = WF._prior_vec(g, prior)
    for k in range(2):
        c = np.linalg.solve(np.asarray(M.todense()), rhs[k])
        assert np.abs(c[alone] - pv[k][alone]).max() <= 1e-12


@pytest.mark.parametrize('cg_max', [1, 3])
def test_pcg_iterate_at_the_cap_is_far_from_converged(cg_max):
    """wind_fit_ref.pcg is CG: run long it meets the direct solve, in fp64 and in long double.  At mu = 1e-2 on the steady 5 x 6 grid
    iterate 1 and iterate 3 are still more than 1e-3 (relative) from the solution, so comparing the kernel's capped cp with them
    says something; the gap between the two precisions at that iterate (printed) is what the GPU test scales its tolerance from; and
    iterations x eps x cond(M) is below 1e-9, which is why the reported residual is held to the true one within 1e-6."""
    g, mu = WF.edge_grid(1, 5, 6), 1e-2
    X = WF.edge_history(3, 4)
    ms = WF.measure(X, 4, WF.EDGE_DT, g, [130, 65, 2], [0.0, 3.0, 7.5], WF.EDGE_W_MAX)
    Hs, bs, _, _ = WF.replay(ms, g, WF.EDGE_W_MAX)
    M, rhs = WF.system(WF.matrix_of(Hs, g), bs, g, WF.EDGE_LAM, mu)
    Md = np.asarray(M.todense())
    assert cg_max * np.finfo(float).eps * np.linalg.cond(Md) < 1e-9
    assert np.finfo(np.longdouble).eps < 1e-3 * np.finfo(float).eps
    for k in range(2):
        sol = np.linalg.solve(Md, rhs[k])
        for ld in (False, True):
            far = WF.pcg(M, rhs[k], np.zeros(30), 200, tol=WF.EDGE_CG_TOL, longdouble=ld)
            assert np.linalg.norm(Md @ far.astype(float) - rhs[k]) <= 2.0 * WF.EDGE_CG_TOL * np.linalg.norm(rhs[k])
            assert np.abs(far.astype(float) - sol).max() <= 1e-6 * np.abs(sol).max()
        x64, xld = WF.pcg(M, rhs[k], np.zeros(30), cg_max), WF.pcg(M, rhs[k], np.zeros(30), cg_max, longdouble=True)
        dist = np.abs(x64 - sol).max() / np.abs(sol).max()
        res = np.linalg.norm(Md @ x64 - rhs[k]) / np.linalg.norm(rhs[k])
        gap = float(np.abs(x64 - xld).max())
        print(f'cg_max = {cg_max}, component {k}: distance from converged {dist:.3e}, residual {res:.3e}, |pcg64 - pcg80| = {gap:.3e}')
        assert dist >= 1e-3 and res > WF.EDGE_CG_TOL and 0.0 < gap <= 1e-12
    # a zero right-hand side from a zero start stays zero; from elsewhere it is solved
    assert not WF.pcg(M, np.zeros(30), np.zeros(30), 5).any()
    assert np.abs(WF.pcg(M, np.zeros(30), np.ones(30), 200)).max() <= 1e-9


def test_zero_right_hand_side_history():
    """psi = 0 and constant y: sincos gives sin(0) = 0 exactly, every m_y is exactly 0, and so is the replayed b[1]."""
    g = WF.edge_grid(1, 5, 6)
    X = WF.zero_rhs_history()
    assert WF.sincos(0.0)[1] == 0.0 and WF.sincos(0.0)[0] == 1.0
    ms = WF.measure(X, 4, WF.EDGE_DT, g, None, None, WF.EDGE_W_MAX)
    assert ms['counts'] == [39 * 4, 0, 0, 0]
    assert not ms['m'][1].any() and np.abs(ms['m'][0] - 2.0).max() <= 1e-11
    _, bs, _, bq = WF.replay(ms, g, WF.EDGE_W_MAX)
    assert not bs[1].any() and not bq[1].any() and bs[0].any()


@pytest.mark.parametrize('origin', [False, True], ids=['box', 'minus-zero'])
def test_sample_edge_case_by_hand(origin):
    """wind_fit_ref.sample_edge_case sample by sample: the reasons, the counts of SAMPLE_EDGE_COUNTS, the segments and weights on the
    box's corners, the measurements on and just above w_max, the scale W."""
    X, g = WF.sample_edge_case(origin)
    assert (g.ny, g.nx) == (5, 6) and WF.SAMPLE_EDGE_DT == 0.0625
    assert [WF.w_pow2(w) for w in (32.0, 33.0, 30.0)] == [32.0, 64.0, 32.0]
    why = {32.0: [[0, 2], [0, -1], [0, 3], [0, 0]], 33.0: [[0, 2], [0, -1], [0, 0], [0, 0]], 30.0: [[0, 2], [0, -1], [3, 3], [0, 0]]}
    for w_max, counts in WF.SAMPLE_EDGE_COUNTS.items():
        ms = WF.measure(X, 1, WF.SAMPLE_EDGE_DT, g, WF.SAMPLE_EDGE_ROWS, None, w_max)
        assert ms['counts'] == counts and ms['why'].T.tolist() == why[w_max]
    # drone 0: exactly the upper corner, used with segment n - 4 and r = 1; then outside
    assert ms['px'][0, 0] == g.x0 + (g.nx - 3) * g.hx and ms['py'][0, 0] == g.y0 + (g.ny - 3) * g.hy
    assert (ms['seg'][1, 0, 0], ms['seg'][2, 0, 0]) == (g.ny - 4, g.nx - 4)
    for b in (ms['bx'][:, 0, 0], ms['by'][:, 0, 0]):
        assert b[0] == 0.0 and b[3] == 1.0 / 6.0 and b[1] == 1.0 / 6.0
    assert ms['px'][1, 0] > g.x0 + (g.nx - 3) * g.hx and list(ms['m'][:, 0, 0]) == [16.0, 16.0]
    # drone 1: exactly the lower corner (origin: through s = -0.0)
    sx, sy = (ms['px'][0, 1] - g.x0) / g.hx, (ms['py'][0, 1] - g.y0) / g.hy
    assert sx == 0.0 and sy == 0.0 and bool(np.signbit(sx)) == origin and bool(np.signbit(sy)) == origin
    assert (ms['seg'][1, 0, 1], ms['seg'][2, 0, 1]) == (0, 0) and ms['bx'][3, 0, 1] == 0.0 and ms['bx'][0, 0, 1] == 1.0 / 6.0
    # drone 2: 32 m/s exactly, then 2^-36 more
    assert list(ms['m'][0, :, 2]) == [32.0, 32.0 + 2.0 ** -36] and not ms['m'][1, :, 2].any()
    # drone 3: headings of -1e6, 1e6, -0.0 at 10 m/s, measurements within every limit used
    assert list(X[:, 2, 3]) == [-1e6, 1e6, 0.0] and np.signbit(X[2, 2, 3]) and np.abs(ms['m'][:, :, 3]).max() < 30.0
    c, s = WF.sincos(X[:, 2, 3])
    assert np.abs(c - np.cos(X[:, 2, 3])).max() <= 4e-16 and np.abs(s - np.sin(X[:, 2, 3])).max() <= 4e-16
