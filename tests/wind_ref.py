"""CPU references of the plant in a wind field (include/d2d.h d2d_wind_field; test infrastructure only).

(a) disc_dyn_glrk_wind: a numpy statement of the kernels' algorithm -- oracle/sim.py's graded or one-panel Gauss mesh per drone, with
    the stage positions solved by fixed-point iteration on the wind term (D2D_WIND_TOL, D2D_WIND_MAX_ITERS).  The kernels stop the
    iteration when every lane of a wavefront has converged, this statement when every drone of the batch has: the two differ at the
    level of the stopping tolerance.
(b) disc_dyn_ivp_wind: the reference's continuous model (src/d2d/dynamic.py:14-28) with field.sample(t, X[:2]) inside the
    right-hand side, integrated by scipy's DOP853 at rtol = atol = 1e-12.

The closed loops reuse oracle/sim.py's controllers unchanged (dcf_get, circle_get, gvf_get, compute_gain, dfff_get) and put (a)
where oracle/sim.py calls disc_dyn_glrk.
"""
import numpy as np
import scipy.integrate

from oracle import sim as S

WIND_TOL, WIND_MAX_ITERS = 1e-13, 8          # include/d2d.h D2D_WIND_*


def _panels_wind(x, y, psi, dphi, dv, phi_c, v_c, field, t, mesh, ns):
    c, b, A = S.gauss_tableau(ns)
    iters = np.zeros(np.shape(x), dtype=np.int64)
    tp = t
    for row in mesh:
        w = row[0]
        vv = np.array([v_c + dv * row[1 + ns + i] for i in range(ns)])
        h = np.array([S.G_ACC * np.tan(phi_c + dphi * row[1 + i]) / vv[i] for i in range(ns)])
        ps = np.array([psi + w * sum(A[i, j] * h[j] for j in range(ns)) for i in range(ns)])
        ax, ay = vv * np.cos(ps), vv * np.sin(ps)
        # stage fixed point: start from the field at the panel's start, at every stage
        w0x, w0y = field.sample_many(tp, x, y)
        ux = np.broadcast_to(w0x, ax.shape).copy(); uy = np.broadcast_to(w0y, ay.shape).copy()
        px = np.array([x + w * sum(A[i, j] * (ax[j] + ux[j]) for j in range(ns)) for i in range(ns)])
        py = np.array([y + w * sum(A[i, j] * (ay[j] + uy[j]) for j in range(ns)) for i in range(ns)])
        tx, ty = WIND_TOL * (1.0 + np.abs(x)), WIND_TOL * (1.0 + np.abs(y))
        done = np.zeros(np.shape(x), dtype=bool)
        for it in range(1, WIND_MAX_ITERS + 1):
            for i in range(ns):
                ux[i], uy[i] = field.sample_many(tp + c[i] * w, px[i], py[i])
            nx = np.array([x + w * sum(A[i, j] * (ax[j] + ux[j]) for j in range(ns)) for i in range(ns)])
            ny = np.array([y + w * sum(A[i, j] * (ay[j] + uy[j]) for j in range(ns)) for i in range(ns)])
            ok = ~(np.abs(nx - px) > tx).any(0) & ~(np.abs(ny - py) > ty).any(0)
            iters = np.where(~done, it, iters)
            done = done | ok
            px, py = nx, ny
            if done.all():
                break
        sx = sum(b[i] * ax[i] for i in range(ns)); sy = sum(b[i] * ay[i] for i in range(ns))
        su = sum(b[i] * ux[i] for i in range(ns)); sv = sum(b[i] * uy[i] for i in range(ns))
        x = x + w * (sx + su); y = y + w * (sy + sv)
        psi = psi + w * sum(b[i] * h[i] for i in range(ns))
        dphi = dphi * row[1 + 2 * ns]; dv = dv * row[2 + 2 * ns]
        tp = tp + w
    return x, y, psi, dphi, dv, iters


def disc_dyn_glrk_wind(Xk, Uk, field, t, dt, tau_phi=0.01, tau_v=1.0, return_iters=False):
    """(a): one plant step from time t in `field` (a d2d.wind.SplineWindField), vectorised over a leading batch axis.  The mesh
    rule per drone is oracle/sim.py disc_dyn_glrk's.  return_iters: also the largest sweep count of each drone's stage solves."""
    Xk = np.asarray(Xk, float); Uk = np.asarray(Uk, float)
    x, y, psi, phi, v = (Xk[..., i].copy() for i in range(5))
    phi_c, v_c = Uk[..., 0], Uk[..., 1]
    dphi = phi - phi_c; dv = v - v_c
    slow = _panels_wind(x, y, psi, dphi, dv, phi_c, v_c, field, t, S.gl_mesh(dt, tau_phi, tau_v), S.GL_STAGES)
    fast = _panels_wind(x, y, psi, dphi, dv, phi_c, v_c, field, t, S.gl_mesh(dt, tau_phi, tau_v, (0.0, 1.0), S.GL_FAST_STAGES),
                        S.GL_FAST_STAGES)
    sel = (np.abs(dphi) <= S.GL_FAST_DPHI) & (dt <= S.GL_FAST_RATIO * tau_phi)
    x, y, psi, dphi, dv, it = (np.where(sel, f, s_) for f, s_ in zip(fast, slow))
    X = np.stack([x, y, S.norm_mpi_pi(psi), phi_c + dphi, v_c + dv], axis=-1)
    return (X, it) if return_iters else X


def disc_dyn_ivp_wind(Xk, Uk, field, t, dt, tau_phi=0.01, tau_v=1.0):
    """(b): one drone, the continuous model with the field sampled inside the right-hand side (src/d2d/dynamic.py:14-28)."""
    def rhs(tt, X):
        return S.cont_dyn(X, tt, Uk, field.sample(tt, X[:2]), tau_phi, tau_v)
    sol = scipy.integrate.solve_ivp(rhs, (t, t + dt), np.asarray(Xk, float), method='DOP853', rtol=1e-12, atol=1e-12)
    X1 = sol.y[:, -1].copy()
    X1[2] = S.norm_mpi_pi(X1[2])
    return X1


def formation_gvf_run_wind(c, r, v_c, X0, n_steps, dt, field, t_start=0.0, ke=4e-4, kd=25.0, kr=20.0, tau_phi=0.01, tau_v=1.0):
    """oracle/sim.py formation_gvf_run (no stop rule) with the plant in `field`: step i from row i - 1 at t_start + (i - 1) dt; the
    guidance law sees no wind.  Returns X (T, n, 5), U (T, n, 2), the largest sweep count."""
    c = np.asarray(c, float); n_ac = c.shape[0]
    B = S.construct_b_matrix(n_ac); z_des = np.zeros(n_ac - 1)
    X = np.zeros((n_steps, n_ac, 5)); U = np.zeros((n_steps, n_ac, 2))
    X[0] = X0
    p = X[0][:, :2].T.copy()
    it_max = 0
    for i in range(1, n_steps):
        U_r, _ = S.dcf_get(B, c, p, z_des, kr)
        Rr = U_r + r
        for j in range(n_ac):
            e, n, H = S.circle_get(X[i - 1, j], c[j], Rr[j])
            Ug, _, _ = S.gvf_get(X[i - 1, j], ke, kd, e, n, H)
            U[i - 1, j] = [np.arctan(Ug / 9.81), v_c]
        X[i], it = disc_dyn_glrk_wind(X[i - 1], U[i - 1], field, t_start + (i - 1) * dt, dt, tau_phi, tau_v, return_iters=True)
        it_max = max(it_max, int(it.max()))
        p = X[i][:, :2].T.copy()
    return X, U, it_max


def track_run_wind(time, x_ref, y_ref, X0s, w, field, tau_phi=0.01, tau_v=1.0):
    """oracle/sim.py track_run with the plant in `field` (step i from row i - 1 at time[i - 1]); the controller keeps the constant w.
    Returns X, U, Xr (T, n, .)."""
    T, n = x_ref.shape
    dt = time[1] - time[0]
    X = np.zeros((T, n, 5)); U = np.zeros((T, n, 2)); Xr = np.zeros((T, n, 5))
    F = [S.compute_derivatives(x_ref[:, j], y_ref[:, j], dt) for j in range(n)]
    X[0] = np.asarray(X0s, float)
    for i in range(1, T):
        for j in range(n):
            Fdx, Fdy, Fddx, Fddy = F[j]
            Xr[i - 1, j], _, U[i - 1, j], _ = S.compute_gain(X[i - 1, j], [x_ref[i, j], y_ref[i, j]], [Fdx[i], Fdy[i]],
                                                             [Fddx[i], Fddy[i]], [0, 0], w, tau_phi, tau_v)
        X[i] = disc_dyn_glrk_wind(X[i - 1], U[i - 1], field, time[i - 1], dt, tau_phi, tau_v)
    return X, U, Xr


def dfff_run_wind(time, Ys, X0, field, perts=None, tau_phi=0.01, tau_v=1.0):
    """oracle/sim.py dfff_run with the plant in `field` and the controller sampling it at the reference point (src/d2d/guidance.py:
    62-65), one aircraft.  Returns X (T, 5), U (T, 2), Xr (T, 5)."""
    T = len(time)
    X = np.zeros((T, 5)); U = np.zeros((T, 2)); Xr = np.zeros((T, 5))
    X[0] = X0
    for i in range(1, T + 1):
        W = field.sample(time[i - 1], Ys[i - 1][0])
        U[i - 1], _, Xr[i - 1] = S.dfff_get(X[i - 1], Ys[i - 1], W, tau_phi, tau_v)
        if i == T:
            break
        X[i] = disc_dyn_glrk_wind(X[i - 1], U[i - 1], field, time[i - 1], time[i] - time[i - 1], tau_phi, tau_v)
        if perts is not None:
            X[i] += perts[i]
    return X, U, Xr


# ---- the three fields of the tests (all smooth, gradients <= ~0.2 /s) ----------------------------------------------------------
def shear(t, x, y):
    """A linear shear layer: wx grows with y, a weak cross component."""
    return 2.0 + 0.02 * y, 0.5 - 0.01 * x


def vortex(t, x, y, xc=10.0, yc=-40.0, gamma=600.0, rc=60.0):
    """A Gaussian (Lamb-Oseen-like) vortex around (xc, yc)."""
    dx, dy = x - xc, y - yc
    r2 = dx * dx + dy * dy
    k = gamma / (2 * np.pi) * (1.0 - np.exp(-r2 / rc ** 2)) / np.maximum(r2, 1e-9)
    k = np.where(r2 < 1e-6, gamma / (2 * np.pi * rc ** 2), k)
    return -k * dy, k * dx


def gust(t, x, y, t_peak=6.0, amp=4.0):
    """A gust front travelling in x, growing and decaying in time (strongest at t_peak)."""
    a = amp * np.exp(-((t - t_peak) / 3.0) ** 2)
    return 1.0 + a * np.exp(-((x - 5.0 * t) / 60.0) ** 2), -0.5 * a * np.sin(y / 50.0)


class FnField:
    """A plain Python field with sample(t, loc): the kind of user class the reference's WindField plug-point takes."""

    def __init__(self, fn):
        self.fn = fn

    def sample(self, t, loc):
        wx, wy = self.fn(t, np.asarray(loc[0], float), np.asarray(loc[1], float))
        return np.array([float(wx), float(wy)])


def spline_of(fn, box=(-150.0, 150.0, -200.0, 150.0), h=10.0, t=None):
    """The SplineWindField that interpolates fn on a uniform grid of spacing h over box = (x0, x1, y0, y1) (and times t)."""
    from d2d.wind import SplineWindField
    x = np.arange(box[0], box[1] + 0.5 * h, h); y = np.arange(box[2], box[3] + 0.5 * h, h)
    if t is None:
        X, Y = np.meshgrid(x, y)
        wx, wy = fn(0.0, X, Y)
        return SplineWindField.from_samples(x, y, wx, wy)
    T, Y, X = np.meshgrid(t, y, x, indexing='ij')
    wx, wy = fn(T, X, Y)
    return SplineWindField.from_samples(x, y, wx, wy, t=t)
