"""CPU: the wind-field spline (d2d/wind.py), its C layout, the unknown-field rule and the two CPU references of the plant in a
field (tests/wind_ref.py: (a) the kernels' algorithm, (b) the reference's continuous model under DOP853)."""
import ctypes
import os
import re

import numpy as np
import pytest

import wind_ref as R
from oracle import sim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_field(steady=True):
    from d2d.wind import SplineWindField
    x = np.linspace(-60.0, 90.0, 16); y = np.linspace(-40.0, 60.0, 11); t = np.linspace(0.0, 8.0, 9)
    rng = np.random.default_rng(2)
    if steady:
        wx, wy = rng.normal(size=(len(y), len(x))), rng.normal(size=(len(y), len(x)))
        return SplineWindField.from_samples(x, y, wx, wy), x, y, None, wx, wy
    wx, wy = rng.normal(size=(len(t), len(y), len(x))), rng.normal(size=(len(t), len(y), len(x)))
    return SplineWindField.from_samples(x, y, wx, wy, t=t), x, y, t, wx, wy


@pytest.mark.parametrize('steady', [True, False])
def test_from_samples_interpolates(steady):
    f, x, y, t, wx, wy = _grid_field(steady)
    if steady:
        Y, X = np.meshgrid(y, x, indexing='ij')
        ex, ey = f.sample_many(0.0, X, Y)
    else:
        T, Y, X = np.meshgrid(t, y, x, indexing='ij')
        ex, ey = f.sample_many(T, X, Y)
    assert np.abs(ex - wx).max() <= 1e-12 and np.abs(ey - wy).max() <= 1e-12      # measured 2e-15
    assert f.cp.shape == ((1,) if steady else (len(t) + 2,)) + (2, len(y) + 2, len(x) + 2)


def test_spline_is_c2_across_knots():
    """One-sided finite differences of value, slope and curvature on both sides of interior knots agree to the difference error."""
    f, x, y, t, _, _ = _grid_field(False)
    for axis, knots in ((0, x[2:-2]), (1, y[2:-2]), (2, t[2:-2])):
        def g(u):
            p = [17.3, -3.1, 2.7]
            p[axis] = u
            return np.array(f.sample_many(p[2], p[0], p[1])).ravel()
        jump, curv = {}, 0.0
        for h in (1e-3, 1e-4):
            jump[h] = 0.0
            for k in knots[::3]:
                L = [g(k - j * h) for j in range(3)]; Rr = [g(k + j * h) for j in range(3)]
                assert np.abs(L[0] - Rr[0]).max() <= 1e-12
                dl, dr = (3 * L[0] - 4 * L[1] + L[2]) / (2 * h), (-3 * Rr[0] + 4 * Rr[1] - Rr[2]) / (2 * h)
                assert np.abs(dl - dr).max() <= 1e-4                               # O(h^2) one-sided slopes
                cl, cr = (L[0] - 2 * L[1] + L[2]) / h ** 2, (Rr[0] - 2 * Rr[1] + Rr[2]) / h ** 2
                jump[h] = max(jump[h], np.abs(cl - cr).max()); curv = max(curv, np.abs(cl).max())
        # The one-sided curvatures differ by O(h |f'''|) for a C2 spline and by the curvature jump itself, O(|f''|), for a C1 one.
        # Measured at h = 1e-3: jump / max |f''| = 1.8e-4 (x), 7.4e-5 (y), 5.2e-4 (t); and it shrinks tenfold with h.
        assert jump[1e-3] <= 1e-3 * curv, (axis, jump, curv)
        assert jump[1e-4] <= 0.2 * jump[1e-3], (axis, jump)


def test_from_field_reproduces_cubic_polynomials():
    from d2d.wind import SplineWindField
    poly = lambda t, x, y: (0.3 + 1e-3 * x ** 3 - 2e-4 * x * y ** 2 + 0.01 * t ** 2 * y - 1e-3 * t ** 3,     # noqa: E731
                            -0.2 + 5e-4 * y ** 3 + 0.002 * x * y * t - 1e-4 * x ** 2)
    lin = lambda t, x, y: (0.3 + 0.01 * x - 0.02 * y + 0.05 * t, -0.2 + 0.03 * y + 0.001 * t)             # noqa: E731
    x = np.linspace(-20.0, 20.0, 9); y = np.linspace(-10.0, 30.0, 9); t = np.linspace(0.0, 6.0, 7)
    rng = np.random.default_rng(4)
    px, py, pt = rng.uniform(-20, 20, 200), rng.uniform(-10, 30, 200), rng.uniform(0, 6, 200)
    # A cubic B-spline reproduces every polynomial of degree <= 3 that its end conditions admit.  The natural ones (second derivative
    # zero at the end knots) admit those whose second derivative vanishes at both ends -- degree <= 1 -- which it reproduces
    # everywhere; a general cubic field is reproduced at every grid point (and between them up to the end effect of the natural
    # conditions, which the interpolation does not claim to remove).
    f = SplineWindField.from_field(R.FnField(lin), x, y, t)
    ex, ey = f.sample_many(pt, px, py)
    wx, wy = lin(pt, px, py)
    assert np.abs(ex - wx).max() <= 1e-12 and np.abs(ey - wy).max() <= 1e-12
    g = SplineWindField.from_field(R.FnField(poly), x, y, t)
    T, Y, X = np.meshgrid(t, y, x, indexing='ij')
    ex, ey = g.sample_many(T, X, Y)
    wx, wy = poly(T, X, Y)
    assert np.abs(ex - wx).max() <= 1e-12 and np.abs(ey - wy).max() <= 1e-12
    # steady: tabulated at t = 0
    h = SplineWindField.from_field(R.FnField(lin), x, y)
    assert h.steady and np.abs(np.array(h.sample(5.0, [3.0, 4.0])) - np.array(lin(0.0, 3.0, 4.0))).max() <= 1e-12


def test_clamped_outside_the_box():
    f, x, y, t, _, _ = _grid_field(True)
    inside = np.array(f.sample(0.0, [x[-1], y[0]]))
    assert np.array_equal(np.array(f.sample(0.0, [x[-1] + 500.0, y[0] - 1e6])), inside)
    assert np.all(np.isfinite(f.sample(0.0, [np.nan, np.inf])))


def test_unknown_field_raises():
    import d2d.guidance as ddg
    import d2d.utils as ddu
    from d2d.wind import SplineWindField, plant_wind
    import full_sim as fs

    class Gusty(ddg.WindField):
        def sample(self, t, loc):
            return [1.0 + 0.1 * t, 0.0]

    assert plant_wind(None) is None and plant_wind(ddg.WindField([1.0, 2.0])) is None and plant_wind(ddu.WindField()) is None
    f = R.spline_of(R.shear)
    assert plant_wind(f) is f and isinstance(f, SplineWindField)
    for bad in (Gusty(), R.FnField(R.vortex)):
        with pytest.raises(NotImplementedError, match='SplineWindField.from_field'):
            plant_wind(bad)
        time = np.arange(0, 1.0, 0.05)
        with pytest.raises(NotImplementedError, match='SplineWindField.from_field'):
            fs.run_simulation_batch(time, np.zeros((len(time), 1, 3, 2)), np.zeros((1, 5)), windfield=bad)
        with pytest.raises(NotImplementedError, match='SplineWindField.from_field'):
            fs.implement_controller_batch(time, np.zeros((len(time), 1)), np.zeros((len(time), 1)), (0, 0), np.zeros((1, 5)), windfield=bad)
        with pytest.raises(NotImplementedError, match='SplineWindField.from_field'):
            fs.CircularFormationGVF_batch(np.zeros((1, 4, 2)), 60.0, 15.0, 4, t_end=1.0, windfield=bad)


def test_wind_field_struct_matches_header():
    import d2dhip
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    body = re.search(r'typedef struct \{([^{}]*)\} d2d_wind_field;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    n_i32 = sum(len(d.split(',')) for d in re.findall(r'int32_t ([^;]+);', body))
    n_f64 = sum(len(d.split(',')) for d in re.findall(r'^\s*double ([^;]+);', body, re.M))
    n_ptr = len(re.findall(r'\*\s*\w+;', body))
    assert (n_i32, n_f64, n_ptr) == (4, 6, 1)
    assert ctypes.sizeof(d2dhip.WindFieldC) == 4 * n_i32 + 8 * n_f64 + 8 * n_ptr == 72
    assert [n for n, _ in d2dhip.WindFieldC._fields_] == ['nt', 'ny', 'nx', 'pad', 't0', 'ht', 'x0', 'hx', 'y0', 'hy', 'cp']
    val = lambda name: float(re.search(r'#define %s ([-+0-9.eE]+)' % name, hdr).group(1))       # noqa: E731
    assert (d2dhip.WIND_TOL, d2dhip.WIND_MAX_ITERS) == (R.WIND_TOL, R.WIND_MAX_ITERS) == (val('D2D_WIND_TOL'), val('D2D_WIND_MAX_ITERS'))


@pytest.mark.parametrize('tau_phi', [0.01, 0.9667])
def test_reference_a_matches_continuous_model_b(tau_phi):
    """(a) -- the kernels' algorithm -- against (b) -- DOP853 on the reference's model with the field inside the right-hand side --
    per step, on both mesh branches (one panel near the bank command, graded panels away from it) and in all three fields."""
    rng = np.random.default_rng(7)
    n = 16
    X = np.stack([rng.uniform(-100, 100, n), rng.uniform(-150, 100, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.7, 0.7, n),
                  rng.uniform(8, 16, n)], 1)
    dphi = np.where(np.arange(n) % 2 == 0, rng.uniform(-S.GL_FAST_DPHI, S.GL_FAST_DPHI, n), rng.uniform(-0.5, 0.5, n))
    U = np.stack([X[:, 3] - dphi, rng.uniform(9, 16, n)], 1)
    for fn, tt in ((R.shear, None), (R.vortex, None), (R.gust, np.arange(0.0, 20.01, 0.5))):
        f = R.spline_of(fn, t=tt)
        Xa, it = R.disc_dyn_glrk_wind(X, U, f, 3.3, 0.05, tau_phi, 1.0, return_iters=True)
        Xb = np.array([R.disc_dyn_ivp_wind(X[i], U[i], f, 3.3, 0.05, tau_phi, 1.0) for i in range(n)])
        d = Xa - Xb; d[:, 2] = S.norm_mpi_pi(d[:, 2])
        assert np.abs(d).max() <= 2e-9, np.abs(d).max()                           # measured 7.8e-10 (tau_phi 0.01), 3e-14 (0.9667)
        assert it.max() <= 6                                                      # measured 4
        # and the field matters: the same step in the wind frozen at the start differs by ~w |grad w| dt^2
        Xc = S.disc_dyn_glrk(X, U, f.sample_many(3.3, X[:, 0], X[:, 1]), 0.05, tau_phi, 1.0)
        assert np.abs(Xc[:, :2] - Xa[:, :2]).max() > 1e-5
