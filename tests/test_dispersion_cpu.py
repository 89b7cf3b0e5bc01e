"""CPU: the statement of d2d_track_dispersion (tests/dispersion_ref.py, ABI 128) against a closed form, its invariants and an
independent second evaluation, and the argument checks of the entry point and of its binding (no GPU: every refusal comes before
the first HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg

import dispersion_ref as D
from oracle import sim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.05
EINVAL = -1                                # include/d2d.h D2D_EINVAL


def _numbers(sigma=1.5, tau=2.0, dt=DT):
    from d2d.wind import GustModel
    return GustModel(sigma, tau=tau).numbers(dt)


def test_straight_reference_converges_to_the_discrete_lyapunov_solution():
    """On a straight, level reference K and F are constant: S tends to the solution of S = F S F^T + Q."""
    k = _numbers()
    v, th = 14.0, 0.4
    Xr, _, _, K = S.compute_gain(np.zeros(5), [0, 0], [v * np.cos(th), v * np.sin(th)], [0, 0], [0, 0])
    Ad, Bd, Ed = D.zoh(*D.plant_jac(Xr), DT)
    F = np.zeros((7, 7)); F[:5, :5] = Ad - Bd @ K; F[:5, 5:] = Ed; F[5, 5] = F[6, 6] = k['a']
    Q = np.zeros((7, 7)); Q[5, 5] = Q[6, 6] = k['s'] ** 2
    rho = np.abs(np.linalg.eigvals(F)).max()
    assert rho < 1.0
    T = int(np.ceil(np.log(1e-14) / (2 * np.log(rho)))) + 2
    assert T < 4000, (rho, T)
    t = np.arange(T) * DT
    got = D.dispersion(v * np.cos(th) * t, v * np.sin(th) * t, DT, k['a'], k['s'], k['sigma'], K=np.tile(K, (T, 1, 1)))
    want = scipy.linalg.solve_discrete_lyapunov(F, Q)
    err = np.abs(D.unpack(got['S']) - want).max() / np.abs(want).max()
    print('rows', T, 'spectral radius', rho, 'relative difference to the Lyapunov solution', err)
    assert err <= 1e-10


def test_invariants_gust_block_symmetry_psd_and_sigma_zero():
    k = _numbers()
    x, y = D.references(3, 60, DT)
    edges = np.array([[1.0, 0.0, 500.0, 0.1], [0.0, 0.0, 0.0, 0.0]])
    discs = np.array([[400.0, 300.0, 10.0]])
    for d in range(3):
        o = D.dispersion(x[:, d], y[:, d], DT, k['a'], k['s'], k['sigma'], edges=edges, discs=discs)
        for row in o['S_hist']:
            Sm = D.unpack(row)
            assert np.abs(Sm[5:, 5:] - k['sigma'] ** 2 * np.eye(2)).max() <= 1e-13 * k['sigma'] ** 2          # the gust stays stationary
            assert np.array_equal(Sm, Sm.T) and np.linalg.eigvalsh(Sm).min() >= -1e-13 * np.abs(Sm).max()
        assert o['fence_row'][1] == -1 and o['fence_k'][1] == np.inf and o['fence_sn'][1] == 0.0                # the absent edge
        assert np.isfinite(o['fence_k'][0]) and np.isfinite(o['disc_k'][0]) and o['sig_max'] > 0
        z = D.dispersion(x[:, d], y[:, d], DT, k['a'], 0.0, 0.0, edges=edges, discs=discs)
        assert not z['S_hist'].any() and z['sig_max'] == 0.0
        assert z['fence_k'][0] == np.inf and z['disc_k'][0] == np.inf and z['fence_row'][0] == 1 and z['disc_row'][0] == 1


def test_second_evaluation_in_long_double_sets_the_floor():
    """dispersion against dispersion_ld on the references of the GPU parity test, with and without a start covariance: the largest
    relative difference is the floor, held under dispersion_ref.CPU_FLOOR (ten times which is the GPU tolerance)."""
    k = _numbers()
    rng = np.random.default_rng(3)
    worst = 0.0
    for T in (2, 3, 40):
        x, y = D.references(9, T, DT)
        for d in range(9):
            _, K = D.reference_gains(x[:, d], y[:, d], DT)
            L = rng.normal(size=(7, 7)) * np.array([0.5, 0.5, 0.02, 0.02, 0.2, 1.0, 1.0])[:, None]
            for S0 in (None, D.pack(L @ L.T)):
                a = D.dispersion(x[:, d], y[:, d], DT, k['a'], k['s'], k['sigma'], K=K, S0=S0)
                b = D.dispersion_ld(x[:, d], y[:, d], DT, k['a'], k['s'], k['sigma'], K=K, S0=S0)
                worst = max(worst, D.rel_err(a['S_hist'], b['S_hist']))
    print('largest relative difference between the two evaluations', worst, 'CPU_FLOOR', D.CPU_FLOOR)
    assert 0.1 * D.CPU_FLOOR <= worst <= D.CPU_FLOOR


def test_two_rows_use_the_first_difference():
    x, y = np.array([0.0, 0.7]), np.array([1.0, 1.2])
    Fdx, Fdy, Fddx, Fddy = D.derivatives(x, y, DT)
    assert np.allclose(Fdx, 0.7 / DT) and np.allclose(Fdy, 0.2 / DT) and not Fddx.any() and not Fddy.any()


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_version_and_declaration():
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 128
    assert 'd2d_track_dispersion' in hdr and 'tests/dispersion_ref.py' in hdr
    import d2dhip
    assert 'd2d_track_dispersion' in d2dhip.EXPORTS and d2dhip.load().d2d_version() >= 128
    assert C.sizeof(d2dhip.DispersionIn) == 4 * 8 and C.sizeof(d2dhip.DispersionOut) == 9 * 8


def test_entry_point_refuses_before_any_hip_call():
    """A zeroed block stands for the context: the checks read none of it, and nothing after them is reached."""
    import d2dhip
    lib = d2dhip.load()
    fake = (C.c_char * 256)()
    buf = (C.c_double * 8)()
    res = D.entry_point_refusals(lib, C.cast(fake, C.c_void_p), C.cast(buf, C.c_void_p))
    assert len(res) >= 20
    for name, rc in res:
        assert rc == EINVAL, (name, rc)
    assert D.entry_point_call(lib, None, d2dhip.Context.track_params(4, 5, DT), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p),
                 d2dhip.DispersionIn(0.9, 0.1, 0.3, None), None, None, d2dhip.DispersionOut()) == EINVAL


def test_binding_argument_checks_raise():
    import d2dhip
    from d2d.wind import GustModel
    td = d2dhip.Context.track_dispersion
    with pytest.raises(TypeError, match='gust model'):
        td(None, None, None, gust=None, dt=DT)
    with pytest.raises(TypeError, match='gust model'):
        td(None, None, None, gust=0.3, dt=DT)
    with pytest.raises(ValueError, match='time= or its step'):
        td(None, None, None, gust=GustModel(0.3, tau=2.0))
    with pytest.raises(ValueError, match='time= or its step'):
        td(None, None, None, gust=GustModel(0.3, tau=2.0), time=np.arange(3.0), dt=DT)


def test_full_sim_refusals_and_margin():
    """full_sim.track_dispersion refuses what the prediction does not cover, by name, before it touches a device;
    dispersion_margin is z_prob times the predicted standard deviations."""
    import full_sim as FS
    from d2d.wind import GustModel, SplineWindField
    from scipy.stats import norm
    t = np.arange(5) * DT
    x = np.zeros((5, 2))
    g = GustModel(0.3, tau=2.0)
    fld = SplineWindField.__new__(SplineWindField)
    with pytest.raises(NotImplementedError, match='SplineWindField'):
        FS.track_dispersion(t, x, x, (0., 0.), g, windfield=fld)
    with pytest.raises(NotImplementedError, match='GVF'):
        FS.track_dispersion(t, x, x, (0., 0.), g, loop='gvf')
    with pytest.raises(NotImplementedError, match='dfff_run'):
        FS.track_dispersion(t, x, x, (0., 0.), g, loop='dfff')
    with pytest.raises(TypeError, match='gust model'):
        FS.track_dispersion(t, x, x, (0., 0.), None)
    rep = dict(gust=GustModel(0.3, tau=2.0, form_corr=0.25), sig_max=np.array([0.5, 0.25]), fence_sn=np.array([[0.4, 0.2]]))
    with pytest.raises(NotImplementedError, match='form_corr'):
        FS.dispersion_margin(rep, 1.35e-3, pair=(0, 1))
    m = FS.dispersion_margin(rep, 1.35e-3)                      # per aircraft: allowed with any form_corr
    z = norm.isf(1.35e-3)
    assert abs(z - 3.0) < 2e-3
    assert abs(m['z'] - z) <= 1e-9
    assert np.allclose(m['fence'], z * rep['fence_sn']) and np.allclose(m['disc'], z * rep['sig_max'])
    rep['gust'] = g
    mp = FS.dispersion_margin(rep, 1.35e-3, pair=(0, 1))
    assert np.isclose(mp['pair'], z * np.sqrt(0.5 ** 2 + 0.25 ** 2))
    for bad in (0.0, 0.5, 1.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='prob'):
            FS.dispersion_margin(rep, bad)
