"""Wind fields that vary in space and time (include/d2d.h d2d_wind_field).

The reference's plant samples its wind field at the aircraft's own position and time on every right-hand-side evaluation
(src/d2d/dynamic.py:14-16, 25-28); the only field it ships, WindField, is constant, and `sample(t, loc)` is the plug-point for a
user's shear, vortex or gust.  The device loops cannot call back into Python, so a field reaches them as a uniform tensor-product
cubic B-spline (C2: the Gauss panels of the plant step keep their order):

  SplineWindField.from_samples(x, y, wx, wy, t=None)  the spline that interpolates gridded samples (natural end conditions)
  SplineWindField.from_field(field, x, y, t=None)     tabulates any object with sample(t, loc) on a grid and fits it
  SplineWindField.sample(t, loc)                      a numpy evaluation of the SAME spline the kernels evaluate: host code and
                                                      device loops see one field
  SplineWindField.derivatives(t, x, y)                value, spatial Jacobian and second derivatives (the collocation planner's
                                                      constraint Jacobian and curvature; sim_device.h wind_eval2 in numpy)
  SplineWindField.sample_num / sample_sym / -field    the planner's wind protocol (src/d2d/opty_utils.py:16-29) and the field with the
                                                      opposite sign (the planner's model has the wind with the opposite sign to the plant)
  GustModel(sigma, tau | L, V, seed, form_corr)       a stochastic gust on top of either wind, drawn inside the device loops
  WindEstimator(x, y, t, lam, mu, w_max, prior).fit   the field fitted to a flown state history on the device (d2d_wind_fit): every
                                                      aircraft is a moving anemometer; WindEstimate is what it returns

Outside the spline's box every coordinate is clamped: the field is held at its boundary value, continuous but only C0 there.
"""
import weakref

import numpy as np
import scipy.linalg

import d2dhip


def _axis_system(n):
    """Banded (2, 2) matrix of the interpolation along one axis with n control points and n - 2 samples: row 0 and row n-1 are the
    natural end conditions (second derivative zero at the first and the last knot), row m + 1 is the spline's value at knot m."""
    ab = np.zeros((5, n))
    def put(i, j, v):
        ab[2 + i - j, j] = v
    put(0, 0, 1.0); put(0, 1, -2.0); put(0, 2, 1.0)
    for i in range(1, n - 1):
        put(i, i - 1, 1.0 / 6.0); put(i, i, 4.0 / 6.0); put(i, i + 1, 1.0 / 6.0)
    put(n - 1, n - 3, 1.0); put(n - 1, n - 2, -2.0); put(n - 1, n - 1, 1.0)
    return ab


def _fit_axis(vals, axis):
    """Control points along `axis` of the spline that interpolates vals (samples along that axis)."""
    v = np.moveaxis(np.asarray(vals, dtype=np.float64), axis, 0)
    m = v.shape[0]
    rhs = np.zeros((m + 2,) + v.shape[1:])
    rhs[1:-1] = v
    c = scipy.linalg.solve_banded((2, 2), _axis_system(m + 2), rhs.reshape(m + 2, -1)).reshape(rhs.shape)
    return np.moveaxis(c, 0, axis)


def _grid(u, name):
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    if len(u) < 2:
        raise ValueError(f'{name}: at least two samples per axis')
    h = u[1] - u[0]
    if not h > 0 or not np.allclose(np.diff(u), h, rtol=1e-9, atol=0.0):
        raise ValueError(f'{name}: the sample grid must be uniform and increasing')
    return float(u[0]), float(h)


def _weights(u, u0, h, n):
    """Segment index and the four uniform cubic B-spline weights of coordinate(s) u (include/d2d.h; sim_device.h wind_axis)."""
    s = (np.asarray(u, dtype=np.float64) - u0) / h
    s = np.where(np.isnan(s), 0.0, np.clip(s, 0.0, n - 3.0))
    fl = np.minimum(np.floor(s), n - 4.0)
    r = s - fl
    q = 1.0 - r; r2 = r * r; r3 = r2 * r
    b = np.stack([q * q * q * (1.0 / 6.0), (3.0 * r3 - 6.0 * r2 + 4.0) * (1.0 / 6.0),
                  (-3.0 * r3 + 3.0 * r2 + 3.0 * r + 1.0) * (1.0 / 6.0), r3 * (1.0 / 6.0)])
    return fl.astype(np.int64), b


def _weights_d(u, u0, h, n):
    """_weights plus the derivative weights B_k'(r) / h and B_k''(r) / h^2.  Along a clamped coordinate (a query outside the box, or
    NaN) both are zero: they are the derivatives of the clamped field."""
    fl, b = _weights(u, u0, h, n)
    s = (np.asarray(u, dtype=np.float64) - u0) / h
    inside = (s >= 0.0) & (s <= n - 3.0)
    r = np.where(np.isnan(s), 0.0, np.clip(s, 0.0, n - 3.0)) - fl
    q = 1.0 - r; r2 = r * r
    d1 = np.stack([-0.5 * q * q, 1.5 * r2 - 2.0 * r, -1.5 * r2 + r + 0.5, 0.5 * r2]) * np.where(inside, 1.0 / h, 0.0)
    d2 = np.stack([q, 3.0 * r - 2.0, 1.0 - 3.0 * r, r]) * np.where(inside, 1.0 / (h * h), 0.0)
    return fl, b, d1, d2


class _FieldSym:
    """What SplineWindField.sample_sym returns: stands where the reference's symbolic wind expressions stand in the equations of
    motion (src/d2d/opty_utils.py:38-50).  Two printable components, and the field itself for the solver (d2d.opty_utils.Eom)."""

    def __init__(self, field, args='t,x,y'):
        self.field, self._args = field, args

    def __getitem__(self, k):
        return ('wx', 'wy')[k] + f'({self._args})'

    def __len__(self):
        return 2


class SplineWindField:
    """A duck-typed WindField (sample(t, loc), summarize()) that the device loops can fly: control points cp (nt, 2, ny, nx) of a
    uniform cubic B-spline over (x, y) (nt = 1, steady) or (t, x, y) (nt >= 4); knot spacings h*, first knots *0."""

    def __init__(self, cp, x0, hx, y0, hy, t0=0.0, ht=1.0):
        cp = np.asarray(cp, dtype=np.float64)
        if cp.ndim == 3:
            cp = cp[None]
        nt, two, ny, nx = cp.shape
        if two != 2 or nx < 4 or ny < 4 or not (nt == 1 or nt >= 4):
            raise ValueError(f'control points (nt, 2, ny, nx) = {cp.shape}: nx, ny >= 4, nt = 1 or >= 4')
        if not (hx > 0 and hy > 0 and (nt == 1 or ht > 0)):
            raise ValueError('knot spacings must be > 0')
        self.cp = np.ascontiguousarray(cp)
        self.cp.setflags(write=False)
        self.x0, self.hx, self.y0, self.hy = float(x0), float(hx), float(y0), float(hy)
        self.t0, self.ht = float(t0), float(ht)
        self._dev = weakref.WeakKeyDictionary()                                 # Context -> (device control points, WindFieldC)

    @property
    def steady(self):
        return self.cp.shape[0] == 1

    @classmethod
    def from_samples(cls, x, y, wx, wy, t=None):
        """The spline that interpolates wx, wy on the uniform grid x (M), y (K) -- arrays (K, M), indexed [y][x] -- or, with the
        uniform sample times t (T), on (t, y, x) -- arrays (T, K, M).  Natural end conditions along every axis."""
        x0, hx = _grid(x, 'x'); y0, hy = _grid(y, 'y')
        w = np.stack([np.asarray(wx, dtype=np.float64), np.asarray(wy, dtype=np.float64)], axis=-3)   # (.., 2, K, M)
        if t is None:
            if w.shape != (2, len(np.ravel(y)), len(np.ravel(x))):
                raise ValueError(f'steady samples: wx, wy must be (len(y), len(x)), got {w.shape[1:]}')
            c = _fit_axis(_fit_axis(w, 2), 1)[None]
            return cls(c, x0, hx, y0, hy)
        t0, ht = _grid(t, 't')
        if w.shape != (len(np.ravel(t)), 2, len(np.ravel(y)), len(np.ravel(x))):
            raise ValueError(f'unsteady samples: wx, wy must be (len(t), len(y), len(x)), got {w.shape[:1] + w.shape[2:]}')
        c = _fit_axis(_fit_axis(_fit_axis(w, 3), 2), 0)
        return cls(c, x0, hx, y0, hy, t0, ht)

    @classmethod
    def from_field(cls, field, x, y, t=None):
        """Tabulate any object with sample(t, loc) -- or, a planner wind object, sample_num(t, x, y) -- on the grid (t at 0.0 for a steady field) and fit it (from_samples)."""
        x = np.asarray(x, dtype=np.float64).reshape(-1); y = np.asarray(y, dtype=np.float64).reshape(-1)
        ts = [0.0] if t is None else list(np.asarray(t, dtype=np.float64).reshape(-1))
        if hasattr(field, 'sample'):
            at = lambda tk, xi, yj: field.sample(tk, np.array([xi, yj]))          # noqa: E731
        else:                                                                 # (a planner wind object: sample_num(t, x, y), no sample)
            at = field.sample_num
        W = np.array([[[np.asarray(at(tk, xi, yj), dtype=np.float64).reshape(2) for xi in x] for yj in y]
                      for tk in ts])                                          # (T, K, M, 2)
        if t is None:
            return cls.from_samples(x, y, W[0, ..., 0], W[0, ..., 1])
        return cls.from_samples(x, y, W[..., 0], W[..., 1], t=t)

    def sample_many(self, t, x, y):
        """The field at arrays t, x, y (broadcast) -> wx, wy: the evaluation of sim_device.h wind_eval in numpy."""
        t, x, y = np.broadcast_arrays(np.asarray(t, np.float64), np.asarray(x, np.float64), np.asarray(y, np.float64))
        shape = x.shape
        t, x, y = t.reshape(-1), x.reshape(-1), y.reshape(-1)
        nt, _, ny, nx = self.cp.shape
        ix, bx = _weights(x, self.x0, self.hx, nx)
        iy, by = _weights(y, self.y0, self.hy, ny)
        if nt == 1:
            it, bt, kt = np.zeros_like(ix), np.ones((1, len(ix))), 1
        else:
            (it, bt), kt = _weights(t, self.t0, self.ht, nt), 4
        out = np.zeros((2, len(ix)))
        for c in range(kt):
            acc = np.zeros((2, len(ix)))
            for a in range(4):
                s = 0.0
                for b in range(4):
                    s = s + bx[b] * self.cp[it + c, :, iy + a, ix + b].T            # (2, P)
                acc = acc + by[a] * s
            out = out + bt[c] * acc
        return out[0].reshape(shape), out[1].reshape(shape)

    def sample(self, t, loc):
        """WindField.sample(t, loc): [wx, wy] at time t and position loc = (x, y)."""
        wx, wy = self.sample_many(t, loc[0], loc[1])
        return np.array([float(wx), float(wy)])

    def derivatives(self, t, x, y):
        """Value w (2, ...), spatial Jacobian J (2, 2, ...) = d(wx, wy)/d(x, y) and second derivatives H (2, 3, ...) = (xx, xy, yy) of
        each component at arrays t, x, y (broadcast): sim_device.h wind_eval2 in numpy.  The value is sample_many's, sum for sum."""
        t, x, y = np.broadcast_arrays(np.asarray(t, np.float64), np.asarray(x, np.float64), np.asarray(y, np.float64))
        shape = x.shape
        t, x, y = t.reshape(-1), x.reshape(-1), y.reshape(-1)
        nt, _, ny, nx = self.cp.shape
        ix, bx, dx, ddx = _weights_d(x, self.x0, self.hx, nx)
        iy, by, dy, ddy = _weights_d(y, self.y0, self.hy, ny)
        if nt == 1:
            it, bt, kt = np.zeros_like(ix), np.ones((1, len(ix))), 1
        else:
            (it, bt), kt = _weights(t, self.t0, self.ht, nt), 4
        P = len(ix)
        out = np.zeros((6, 2, P))                                                   # value, d/dx, d/dy, xx, xy, yy
        for c in range(kt):
            acc = np.zeros((6, 2, P))
            for a in range(4):
                s = np.zeros((3, 2, P))                                                # row sums: value, d/dx, d2/dx2
                for b in range(4):
                    cpv = self.cp[it + c, :, iy + a, ix + b].T
                    s = s + np.stack([bx[b] * cpv, dx[b] * cpv, ddx[b] * cpv])
                acc = acc + np.stack([by[a] * s[0], by[a] * s[1], dy[a] * s[0], by[a] * s[2], dy[a] * s[1], ddy[a] * s[0]])
            out = out + bt[c] * acc
        w = out[0].reshape((2,) + shape)
        J = np.stack([out[1], out[2]], axis=1).reshape((2, 2) + shape)               # J[k][0] = d w_k / dx, J[k][1] = d w_k / dy
        H = np.stack([out[3], out[4], out[5]], axis=1).reshape((2, 3) + shape)
        return w, J, H

    # ---- the planner's wind protocol (src/d2d/opty_utils.py:16-29: sample_sym inside the equations of motion, sample_num per node)
    def sample_num(self, t, x, y):
        """[wx, wy] at (t, x, y): the same numbers as sample(t, (x, y))."""
        return self.sample(t, (x, y))

    def sample_sym(self, _t, _x, _y):
        """The wind of the symbolic model: a marker that carries this field (d2d.opty_utils.Eom keeps it as eom.field)."""
        return _FieldSym(self)

    def __neg__(self):
        """The field with the opposite sign (control points negated, same knots).  The planner's model adds its wind to the
        RESIDUAL, xdot - v cos(psi) + wx = 0 (the reference's quirk, src/d2d/opty_utils.py:42-44), the plant to the velocity,
        xdot = v cos(psi) + wx (src/d2d/dynamic.py:18-19): a plan consistent with a plant that flies F is planned in -F."""
        return SplineWindField(-self.cp, self.x0, self.hx, self.y0, self.hy, self.t0, self.ht)

    def negated(self):
        """-self, built once and kept: callers that plan in -F for a plant that flies F on every call (full_sim's mission chain) reuse
        one field, and with it its device copy (device_field caches on the field object)."""
        if getattr(self, '_neg', None) is None:
            self._neg = -self
        return self._neg

    def summarize(self):
        nt, _, ny, nx = self.cp.shape
        kind = 'steady' if nt == 1 else f'unsteady, t in [{self.t0:g}, {self.t0 + (nt - 3) * self.ht:g}] s'
        return (f'cubic B-spline wind field ({kind}), x in [{self.x0:g}, {self.x0 + (nx - 3) * self.hx:g}] m, '
                f'y in [{self.y0:g}, {self.y0 + (ny - 3) * self.hy:g}] m, |w| <= {np.abs(self.cp).max():.3g} m/s')

    def __str__(self):
        return self.summarize()

    def device_field(self, ctx):
        """d2dhip.WindFieldC of this field for ctx.  The control points are uploaded once per context and kept while the context
        lives: the cache holds the context weakly, so a long-lived field keeps neither the context nor its device copy alive."""
        hit = self._dev.get(ctx)
        if hit is None:
            cp = ctx.dev(np.array(self.cp))                                        # (a writable copy for torch)
            nt, _, ny, nx = self.cp.shape
            f = d2dhip.WindFieldC(nt, ny, nx, 0, self.t0, self.ht, self.x0, self.hx, self.y0, self.hy, cp.data_ptr())
            hit = (cp, f)
            self._dev[ctx] = hit
        return hit[1]


class GustModel:
    """A stochastic gust of the plant (include/d2d.h d2d_gust): per aircraft and axis a first-order Gauss-Markov process of standard
    deviation sigma (m/s) and correlation time tau (s) -- or tau = L / V, the first-order Dryden form with length scale L (m) at
    airspeed V (m/s) -- of which the fraction form_corr in [0, 1) of the variance is shared by the aircraft of a formation.  It
    holds parameters only: the device loops draw the numbers (Philox4x32-10 on (seed, drone, phase, step)), and the controllers never
    see the gust.  Pass it as gust= to full_sim's batched loops or to Context.gvf_run / track_run / gust_sample."""

    def __init__(self, sigma, tau=None, L=None, V=None, seed=0, form_corr=0.0):
        if (tau is None) == (L is None and V is None) or (tau is None and (L is None or V is None)):
            raise ValueError('give the correlation time as tau, or as the pair L, V (tau = L / V)')
        if tau is None:
            if not (np.isfinite(L) and np.isfinite(V) and L > 0 and V > 0):
                raise ValueError(f'L={L!r}, V={V!r}: both must be finite and > 0')
            tau = float(L) / float(V)
        if not (np.isfinite(sigma) and sigma >= 0):
            raise ValueError(f'sigma={sigma!r} must be finite and >= 0')
        if not (np.isfinite(tau) and tau > 0):
            raise ValueError(f'tau={tau!r} must be finite and > 0')
        if not (np.isfinite(form_corr) and 0.0 <= form_corr < 1.0):
            raise ValueError(f'form_corr={form_corr!r} must be in [0, 1)')
        if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f'seed={seed!r} must be an integer in [0, 2^64)')
        self.sigma, self.tau, self.seed, self.form_corr = float(sigma), float(tau), int(seed), float(form_corr)

    def numbers(self, dt):
        """The numbers the process runs on for a step dt, computed once in fp64: dict(seed, a = exp(-dt / tau),
        s = sigma sqrt(1 - a^2), sigma, w_own = sqrt(1 - c), w_form = sqrt(c))."""
        if not (np.isfinite(dt) and dt > 0):
            raise ValueError(f'dt={dt!r} must be finite and > 0')
        a = float(np.exp(-float(dt) / self.tau))
        return dict(seed=self.seed, a=a, s=self.sigma * float(np.sqrt(1.0 - a * a)), sigma=self.sigma,
                    w_own=float(np.sqrt(1.0 - self.form_corr)), w_form=float(np.sqrt(self.form_corr)))

    def lower(self, dt, n_ac, phase=0, stream_base=0, step_base=0):
        """d2dhip.GustC for a loop of step dt over formations of n_ac aircraft: phase separates the loops of one mission, stream_base
        is the global index of the call's first drone (a multiple of n_ac: a shard's first drone), step_base the steps a continued
        series has already made.  The state and history pointers are the caller's to fill."""
        if int(n_ac) < 1 or int(phase) < 0 or int(stream_base) < 0 or int(stream_base) % int(n_ac) or int(step_base) < 0:
            raise ValueError(f'n_ac={n_ac} >= 1, phase={phase} >= 0, step_base={step_base} >= 0 and stream_base={stream_base} a multiple of n_ac >= 0')
        k = self.numbers(dt)
        return d2dhip.GustC(k['seed'], int(stream_base), int(phase), int(n_ac), int(step_base), k['a'], k['s'], k['sigma'], k['w_own'],
                            k['w_form'], None, None, None)


def plant_gust(gust):
    """A gust= argument of a device loop: None, or a GustModel (anything else cannot be drawn on the device)."""
    if gust is None or isinstance(gust, GustModel):
        return gust
    raise TypeError(f'{type(gust).__name__} is not a gust model: build one with d2d.wind.GustModel(sigma, tau=...)')


class WindEstimate:
    """What WindEstimator.fit returns: the fitted control points on the device with the estimator's geometry.  cp dev
    [nt][2][ny][nx]; support dev [nt ny nx] (diag A^T A: how much data backs each control point); stats dev [8]
    (d2dhip.WINDFIT_STATS).  Nothing here visits the host until field(), stats_host() or rms is asked for."""

    def __init__(self, ctx, res, geom):
        self.ctx, self.cp, self.support, self.stats = ctx, res['cp'], res.get('support'), res.get('stats')
        self._field, self._geom, self._neg = res['field'], geom, None

    def device_field(self, ctx=None):
        """d2dhip.WindFieldC on the fitted control points (this object keeps them alive)."""
        assert ctx is None or ctx is self.ctx, 'the estimate lives on the context that fitted it'
        return self._field

    def negated_device_field(self, ctx=None):
        """A WindEstimate-like field object of -F, negated on the device (the planner's model adds its wind to the residual: a plan
        for a plant that flies F is planned in -F); device_field(ctx) of the result is its WindFieldC."""
        assert ctx is None or ctx is self.ctx, 'the estimate lives on the context that fitted it'
        if self._neg is None:
            cp = (-self.cp).contiguous()
            f = self._field
            self._neg = WindEstimate(self.ctx, dict(cp=cp, support=self.support, stats=self.stats,
                                                    field=d2dhip.WindFieldC(f.nt, f.ny, f.nx, 0, f.t0, f.ht, f.x0, f.hx, f.y0, f.hy, cp.data_ptr())),
                                     self._geom)
        return self._neg

    def field(self):
        """The estimate as a host SplineWindField (synchronises): for Planner(exp) users and for plotting."""
        g = self._geom
        return SplineWindField(self.cp.cpu().numpy(), g['x0'], g['hx'], g['y0'], g['hy'], g['t0'], g['ht'])

    def stats_host(self):
        """dict of the eight numbers of stats (synchronises)."""
        return dict(zip(d2dhip.WINDFIT_STATS, (float(v) for v in self.stats.cpu().numpy())))

    @property
    def rms(self):
        """(rms_x, rms_y) of the fit's residual over the used samples, m/s: about the gust level (synchronises)."""
        s = self.stats_host()
        n = max(s['used'], 1.0)
        return float(np.sqrt(s['rss_x'] / n)), float(np.sqrt(s['rss_y'] / n))


class WindEstimator:
    """Fits a SplineWindField to flown state histories on the device (include/d2d.h d2d_wind_fit).  x, y (and t, None: steady) are
    uniform KNOT grids: the estimate lives on [x[0], x[-1]] x [y[0], y[-1]] (x [t[0], t[-1]]) with len + 2 control points per axis,
    and samples outside that box are rejected.  lam: the weight of the second differences of the control points, one number or
    (lam_x, lam_y, lam_t); mu > 0: the pull towards the prior, which decides the cells no aircraft visited; w_max: measurements above
    it are rejected; prior: a constant (wx, wy) or a SplineWindField on the same grid (None: no wind); rec_stride: the stride at which
    full_sim's loops keep the history they hand to fit (dt_row = t_step rec_stride; the trapezoid error grows with its square)."""

    def __init__(self, x, y, t=None, lam=1e-2, mu=1e-6, w_max=50.0, prior=None, rec_stride=1, cg_tol=1e-10, cg_max=2000):
        self.x0, self.hx = _grid(x, 'x'); self.y0, self.hy = _grid(y, 'y')
        self.nx, self.ny = len(np.ravel(x)) + 2, len(np.ravel(y)) + 2
        self.t0, self.ht, self.nt = 0.0, 1.0, 1
        if t is not None:
            self.t0, self.ht = _grid(t, 't')
            self.nt = len(np.ravel(t)) + 2
        if self.nt * self.ny * self.nx > d2dhip.WINDFIT_MAX_CP:
            raise ValueError(f'x, y, t: {self.nt} x {self.ny} x {self.nx} control points, at most {d2dhip.WINDFIT_MAX_CP}')
        lam3 = (float(lam),) * 3 if np.ndim(lam) == 0 else tuple(float(v) for v in lam)
        if len(lam3) != 3 or not all(np.isfinite(v) and v >= 0 for v in lam3):
            raise ValueError(f'lam={lam!r}: one number or (lam_x, lam_y, lam_t), finite and >= 0')
        if not (np.isfinite(mu) and mu > 0):
            raise ValueError(f'mu={mu!r} must be finite and > 0 (it decides the cells no aircraft visited)')
        if not (np.isfinite(w_max) and w_max > 0):
            raise ValueError(f'w_max={w_max!r} must be finite and > 0')
        if int(rec_stride) != rec_stride or int(rec_stride) < 1:
            raise ValueError(f'rec_stride={rec_stride!r} must be an integer >= 1')
        if not (0 < cg_tol < 1) or int(cg_max) < 1:
            raise ValueError(f'cg_tol={cg_tol!r} in (0, 1) and cg_max={cg_max!r} >= 1 required')
        shape = (self.nt, 2, self.ny, self.nx)
        if prior is None:
            self.prior = None
        elif isinstance(prior, SplineWindField):
            same = prior.cp.shape == shape and np.allclose([prior.x0, prior.hx, prior.y0, prior.hy], [self.x0, self.hx, self.y0, self.hy]) \
                and (self.nt == 1 or np.allclose([prior.t0, prior.ht], [self.t0, self.ht]))
            if not same:
                raise ValueError('prior: a SplineWindField prior must live on the estimator\'s own grid')
            self.prior = np.array(prior.cp)
        else:
            pr = np.asarray(prior, dtype=np.float64).reshape(-1)
            if pr.shape != (2,) or not np.isfinite(pr).all():
                raise ValueError(f'prior={prior!r}: a constant (wx, wy) or a SplineWindField on the same grid')
            self.prior = np.ascontiguousarray(np.broadcast_to(pr[None, :, None, None], shape))
        self.lam, self.mu, self.w_max, self.rec_stride = lam3, float(mu), float(w_max), int(rec_stride)
        self.cg_tol, self.cg_max = float(cg_tol), int(cg_max)
        self._dev = weakref.WeakKeyDictionary()                                 # Context -> device prior

    def geometry(self):
        """The d2d_wind_field geometry of the estimate (SplineWindField's convention: n knots, n + 2 control points, first knot x[0])."""
        return dict(nt=self.nt, ny=self.ny, nx=self.nx, t0=self.t0, ht=self.ht, x0=self.x0, hx=self.hx, y0=self.y0, hy=self.hy)

    def device_field(self, ctx):
        """The geometry as a d2dhip.WindFieldC without control points (what Context.wind_fit takes as its grid)."""
        g = self.geometry()
        return d2dhip.WindFieldC(g['nt'], g['ny'], g['nx'], 0, g['t0'], g['ht'], g['x0'], g['hx'], g['y0'], g['hy'], None)

    def fit(self, ctx, X_hist, n_ac, dt_row, rows=None, t_start=None, outputs=None):
        """X_hist dev [n_rows][5][N] (rows dev int32 [n_form], t_start dev [n_form] or a float as in Context.flight_audit) -> WindEstimate."""
        prior = None
        if self.prior is not None:
            prior = self._dev.get(ctx)
            if prior is None:
                prior = self._dev[ctx] = ctx.dev(self.prior)
        res = ctx.wind_fit(X_hist, n_ac, dt_row, self, rows=rows, t_start=t_start, prior=prior, w_max=self.w_max, lam=self.lam, mu=self.mu,
                           cg_tol=self.cg_tol, cg_max=self.cg_max, outputs=outputs)
        return WindEstimate(ctx, res, self.geometry())


def wind_estimator(wind_estimate):
    """A wind_estimate= argument: None, or a WindEstimator."""
    if wind_estimate is None or isinstance(wind_estimate, WindEstimator):
        return wind_estimate
    raise TypeError(f'{type(wind_estimate).__name__} is not a wind estimator: build one with d2d.wind.WindEstimator(x, y, t)')


def _is_constant_class(cls):
    import d2d.guidance, d2d.utils, d2d.opty_utils      # noqa: E401
    return getattr(cls, 'sample', None) in (None, d2d.guidance.WindField.sample) or cls in (d2d.utils.WindField, d2d.opty_utils.WindField)


def plant_wind(windfield):
    """How a batched device loop flies `windfield`: None / a constant class -> None (the constant-wind path, unchanged);
    a SplineWindField -> the field.  Any other object whose class has its own sample(t, loc) cannot be flown as it is: the loops do
    not call back into Python, and freezing it at one sample would fly a different field silently."""
    if windfield is None or isinstance(windfield, SplineWindField):
        return windfield
    if _is_constant_class(type(windfield)):
        return None
    raise NotImplementedError(
        f'{type(windfield).__name__}.sample varies the wind in space or time and the device loops cannot call it: tabulate it on a '
        f'grid with d2d.wind.SplineWindField.from_field(field, x, y, t) and pass that field instead')


def planner_wind(wind):
    """How the collocation planner plans in `wind`: a constant class (its sample_sym is the reference's, which returns w) -> None
    (the constant-wind path, unchanged); a SplineWindField -> the field.  Any other object whose class has its own sample_sym varies
    the wind inside the equations of motion, which the kernels cannot call: same rule as plant_wind."""
    if wind is None or isinstance(wind, SplineWindField):
        return wind
    import d2d.opty_utils, d2d.utils      # noqa: E401
    if getattr(type(wind), 'sample_sym', None) in (None, d2d.opty_utils.WindField.sample_sym, d2d.utils.WindField.sample_sym):
        return None
    raise NotImplementedError(
        f'{type(wind).__name__}.sample_sym varies the wind in space or time and the planner cannot differentiate it: tabulate it on a '
        f'grid with d2d.wind.SplineWindField.from_field(field, x, y, t) and pass that field instead')
