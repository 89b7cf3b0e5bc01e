"""CPU: the stochastic gusts of the plant (include/d2d.h d2d_gust, ABI 118) as tests/gust_ref.py states them -- the Philox4x32-10
known answers, the moments of the normal pairs, the stationary variance and the autocorrelation of the Gauss-Markov process, the
formation correlation -- and the host side: d2d.wind.GustModel's lowering and refusals, the header and the binding.
Bounds: 4 standard errors of each statistic at the sample size used (measured values beside the asserts)."""
import inspect
import os
import re

import numpy as np
import pytest

import gust_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20241008


def test_philox_known_answers():
    kat = [([0, 0, 0, 0], [0, 0], '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ([0xffffffff] * 4, [0xffffffff] * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for ctr, key, want in kat:
        assert ' '.join('%08x' % int(v) for v in G.philox4x32_10(ctr, key)) == want
    # batched: the three at once
    out = G.philox4x32_10(np.array([k[0] for k in kat]), np.array([k[1] for k in kat]))
    assert [' '.join('%08x' % int(v) for v in row) for row in out] == [k[2] for k in kat]


@pytest.mark.parametrize('phase', [0, 1, 2])
def test_normal_pairs_have_unit_moments(phase):
    """65 536 streams at steps 0, 1, 7, 255: mean 0, variance 1, E[xi_x xi_y] = 0, each within 4 standard errors (2 n samples for the
    first two: se 1 / sqrt(2 n) and sqrt(2 / (2 n)); n products of unit variance for the third: 1 / sqrt(n)).  Measured: <= 2.4."""
    n = 65536
    for step in (0, 1, 7, 255):
        x, y = G.normals(SEED, np.arange(n), phase, 0, step)
        z = np.concatenate([x, y])
        dev = (abs(z.mean()) * np.sqrt(2 * n), abs(z.var() - 1.0) / np.sqrt(2.0 / (2 * n)), abs((x * y).mean()) * np.sqrt(n))
        print(phase, step, dev)
        assert max(dev) <= 4.0, (phase, step, dev)
        assert np.isfinite(z).all()


def test_process_is_stationary_with_the_stated_autocorrelation():
    """4096 streams x 513 rows, dt 0.05, tau 2, sigma 1.5: row std / sigma within 0.039 of 1 at rows 0, 256, 512 (4 se of a standard
    deviation over 8192 samples is 4 / sqrt(2 * 8192) = 0.031; the issue's bound) and corr(row 256, row 296) within 0.044 of a^40
    (4 se of a correlation of 0.37 over 8192 pairs: 4 (1 - 0.37^2) / sqrt(8192) = 0.038)."""
    from d2d.wind import GustModel
    gm = GustModel(1.5, tau=2.0, seed=SEED).numbers(0.05)
    g, gs = G.sample(gm, 4096, 513, 1, 0)
    for r in (0, 256, 512):
        print(r, g[r].std() / 1.5)
        assert abs(g[r].std() / 1.5 - 1.0) <= 0.039                      # measured 0.995 .. 1.014
    rho = np.corrcoef(g[256].ravel(), g[296].ravel())[0, 1]
    print(rho, gm['a'] ** 40)
    assert abs(rho - gm['a'] ** 40) <= 0.044                             # measured 0.371 against 0.368
    assert np.array_equal(g, gs[:, :2]) and not gs[:, 2:].any()          # no shared part: g is the own process, the shared planes stay 0


def test_formation_correlation():
    """Two aircraft of one formation correlate at c = 0.36, aircraft of different formations at 0: 8192 formations of 2, the x and y
    components of row 0 and of row 100 (50 correlation times later: independent) -- 32 768 pairs, se (1 - rho^2) / sqrt(n)."""
    from d2d.wind import GustModel
    c = 0.36
    gm = GustModel(1.0, tau=0.1, seed=SEED, form_corr=c).numbers(0.05)
    g, _ = G.sample(gm, 16384, 101, 2, 1)
    v = np.concatenate([g[0].reshape(2, 8192, 2), g[100].reshape(2, 8192, 2)], 0)      # (4, formation, aircraft)
    a, b = v[:, :, 0].ravel(), v[:, :, 1].ravel()
    n = a.size
    same = np.corrcoef(a, b)[0, 1]
    other = np.corrcoef(a, np.roll(v[:, :, 1], 1, axis=1).ravel())[0, 1]
    print(same, other)
    assert abs(same - c) <= 4 * (1 - c * c) / np.sqrt(n)
    assert abs(other) <= 4 / np.sqrt(n)
    assert abs(g[0].std() - 1.0) <= 4 / np.sqrt(2 * g[0].size)            # the combination keeps sigma


def test_a_continued_series_and_a_sub_range_reproduce_the_whole():
    """(seed, stream, phase, step) alone: rows 32 .. 64 from the state of row 32 with step_base 32, and streams 30 .. 59 on their own."""
    from d2d.wind import GustModel
    gm = GustModel(1.5, tau=2.0, seed=7, form_corr=0.36).numbers(0.05)
    base = 3 * 2 ** 31
    g, gs = G.sample(gm, 129, 65, 3, 2, stream_base=base)
    g2, _ = G.sample(gm, 129, 33, 3, 2, stream_base=base, state=gs[32], step_base=32)
    assert np.array_equal(g2, g[32:])
    g3, _ = G.sample(gm, 30, 65, 3, 2, stream_base=base + 30)
    assert np.array_equal(g3, g[:, :, 30:60])
    # the high stream word is used: the same low words under another high word draw other numbers
    g4, _ = G.sample(gm, 129, 2, 3, 2, stream_base=base - 2 ** 32)
    assert np.abs(g4 - g[:2]).min() > 0


def test_gust_model_lowering_and_refusals():
    import d2dhip
    from d2d.wind import GustModel
    m = GustModel(1.5, tau=2.0, seed=SEED, form_corr=0.36)
    g = m.lower(0.05, 3, phase=2, stream_base=3 * 2 ** 31)
    assert isinstance(g, d2dhip.GustC)
    a = np.exp(-0.05 / 2.0)
    assert g.a == a and g.s == 1.5 * np.sqrt(1.0 - a * a) and g.sigma == 1.5
    assert g.w_own == np.sqrt(1.0 - 0.36) and g.w_form == np.sqrt(0.36) and abs(g.w_own ** 2 + g.w_form ** 2 - 1.0) <= 1e-15
    assert (g.seed, g.stream_base, g.phase, g.n_ac, g.step_base) == (SEED, 3 * 2 ** 31, 2, 3, 0)
    assert g.state_in is None and g.state_out is None and g.g_hist is None
    assert GustModel(1.0, tau=2.0).lower(0.05, 1).w_form == 0.0
    d = GustModel(1.0, L=30.0, V=12.0)                                   # the first-order Dryden form: tau = L / V
    assert d.tau == 2.5 and d.lower(0.1, 4).a == np.exp(-0.1 / 2.5)
    assert GustModel(0.0, tau=1.0).lower(0.05, 1).s == 0.0
    assert GustModel(1.0, tau=1.0, seed=2 ** 64 - 1).lower(0.05, 1).seed == 2 ** 64 - 1
    for kw in (dict(sigma=-1.0, tau=1.0), dict(sigma=np.nan, tau=1.0), dict(sigma=1.0), dict(sigma=1.0, tau=1.0, L=3.0, V=1.0),
               dict(sigma=1.0, L=3.0), dict(sigma=1.0, tau=0.0), dict(sigma=1.0, tau=np.inf), dict(sigma=1.0, L=-1.0, V=2.0),
               dict(sigma=1.0, tau=1.0, form_corr=1.0), dict(sigma=1.0, tau=1.0, form_corr=-0.1), dict(sigma=1.0, tau=1.0, seed=-1),
               dict(sigma=1.0, tau=1.0, seed=1.5)):
        with pytest.raises(ValueError):
            GustModel(**kw)
    for args in ((0.0, 3), (0.05, 0), (0.05, 3, -1), (0.05, 3, 0, 4), (0.05, 3, 0, -3), (0.05, 3, 0, 0, -1)):
        with pytest.raises(ValueError):
            m.lower(*args)


def test_the_header_and_the_binding_carry_the_gust():
    import d2dhip
    import full_sim
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 118
    for fn in ('d2d_gust_sample', 'd2d_sim_gvf_run_gust', 'd2d_sim_track_run_gust'):
        assert fn in d2dhip.EXPORTS and re.search(r'\bint %s\(' % fn, hdr), fn
    body = re.search(r'typedef struct \{([^}]*)\} d2d_gust;', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)).group(1)
    names = [n.strip().lstrip('*') for decl in re.findall(r'(?:const )?(?:uint64_t|int64_t|int32_t|double) ([^;]+);', body) for n in decl.split(',')]
    assert names == [k for k, _ in d2dhip.GustC._fields_]
    for need in ('seed', 'stream_base', 'phase', 'n_ac', 'a', 's', 'sigma', 'w_own', 'w_form', 'state_in', 'state_out', 'g_hist'):
        assert need in names
    # gust=None is the default everywhere: nothing new is launched
    for fn in (full_sim.full_sim_phases_batch, full_sim.CircularFormationGVF_batch, full_sim.implement_controller_batch):
        assert inspect.signature(fn).parameters['gust'].default is None
    for fn in (d2dhip.Context.gvf_run, d2dhip.Context.track_run):
        p = inspect.signature(fn).parameters
        assert p['gust'].default is None and p['gust_state'].default is None and p['gust_phase'].default == 0
    assert callable(d2dhip.Context.gust_sample)


def test_the_planners_take_no_gust():
    import full_sim
    import multi_opt_planner as mop
    import single_opt_planner as sop
    from d2d.wind import GustModel
    m = GustModel(1.0, tau=2.0)
    with pytest.raises(ValueError, match='property of the plant'):
        full_sim.plan_batch(np.zeros((1, 80)), 50, 4.9, 0.1, gust=m)
    with pytest.raises(ValueError, match='property of the plant'):
        full_sim.plan_batch(np.zeros((1, 80)), 50, 4.9, 0.1, backend='nlp', gust=m)
    with pytest.raises(ValueError, match='property of the plant'):
        sop.Planner(None, gust=m)
    with pytest.raises(ValueError, match='property of the plant'):
        mop.Planner(None, gust=m)
    with pytest.raises(TypeError, match='GustModel'):
        full_sim.implement_controller_batch(np.arange(3) * 0.1, np.zeros((3, 1)), np.zeros((3, 1)), (0., 0.), np.zeros((1, 5)), gust=1.0)


def test_shards_fly_the_gusts_of_the_whole_batch():
    from d2dhip import dist
    from d2d.wind import GustModel
    gm = GustModel(1.0, tau=1.0, seed=3, form_corr=0.25).numbers(0.05)
    n_form, n_ac, world = 7, 3, 3
    whole, _ = G.sample(gm, n_form * n_ac, 9, n_ac, 1)
    for rank in range(world):
        lo, hi = dist.shard_bounds(n_form, rank, world)
        base = dist.gust_stream_base(n_form, rank, world, n_ac)
        assert base == lo * n_ac
        part, _ = G.sample(gm, (hi - lo) * n_ac, 9, n_ac, 1, stream_base=base)
        assert np.array_equal(part, whole[:, :, lo * n_ac:hi * n_ac])


def test_the_loops_of_the_statement_stand_on_the_oracle_and_on_wind_ref():
    """gust_ref's plant step in a field is wind_ref's with the gust added to every value read (random states on both meshes, a
    steady and an unsteady field, a start time per drone); with sigma = 0 its closed loops are oracle/sim.py's, bit for bit."""
    import wind_ref as R
    from oracle import sim as S
    from d2d.wind import GustModel
    rng = np.random.default_rng(3); n = 256
    X = np.stack([rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(-3.1, 3.1, n), rng.uniform(-.7, .7, n), rng.uniform(8, 16, n)], 1)
    dphi = np.where(rng.random(n) < .5, rng.uniform(-S.GL_FAST_DPHI, S.GL_FAST_DPHI, n), rng.uniform(-.5, .5, n))
    U = np.stack([X[:, 3] - dphi, rng.uniform(9, 16, n)], 1)
    g = rng.normal(size=(2, n)) * 1.5
    for f, t in ((R.spline_of(R.vortex), 4.2), (R.spline_of(R.gust, t=np.arange(0, 30.01, .5)), rng.uniform(1, 9, n))):
        for tau in (0.01, 0.9667):
            a = G.disc_dyn_glrk_gust(X, U, f, g, t, 0.05, tau, 1.0)
            b = R.disc_dyn_glrk_wind(X, U, G._Offset(f, g), t, 0.05, tau, 1.0)
            d = a - b; d[:, 2] = S.norm_mpi_pi(d[:, 2])
            assert np.abs(d).max() <= 1e-10                              # (the sweeps' stopping tolerance; measured 0.0)
            assert np.abs(a[:, :2] - R.disc_dyn_glrk_wind(X, U, f, t, 0.05, tau, 1.0)[:, :2]).max() > 1e-3      # and the gust is in it
    calm = GustModel(0.0, tau=2.0).numbers(0.05)
    c = np.array([[0, -20], [25, -40], [25, -80.0]]); X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (3, 1))
    Xz, Uz, Gz, stop, gs = G.formation_gvf_run_gust(c, 60.0, 15.0, X0, 61, 0.05, calm, 0, n_form=2, W=(0.5, -0.3))
    Xs, Us, *_ = S.formation_gvf_run(c, 60.0, 15.0, X0, 61, 0.05, W=(0.5, -0.3))
    assert np.array_equal(Xz[:, 0], Xs) and np.array_equal(Xz[:, 1], Xs) and np.array_equal(Uz[:, 0], Us) and not Gz.any() and not gs.any()
    time = np.arange(21) * 0.1
    xr = (12.0 * time)[:, None] + np.zeros((1, 2)); yr = np.sin(0.3 * time)[:, None] * np.array([[1.0, -2.0]])
    X0t = np.array([[0.5, -1.0, 0.05, 0.0, 11.5], [-0.5, 1.0, -0.05, 0.0, 12.5]])
    Xa, Ua, Xra, _, _ = G.track_run_gust(time, xr, yr, X0t, (0.5, -0.3), GustModel(0.0, tau=2.0).numbers(0.1), 1)
    Xb, Ub, Xrb, *_ = S.track_run(time, xr, yr, X0t, (0.5, -0.3))
    assert np.array_equal(Xa, Xb) and np.array_equal(Ua[:-1], Ub[:-1])
