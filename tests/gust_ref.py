"""CPU statement of the stochastic gusts (include/d2d.h d2d_gust; test infrastructure only): Philox4x32-10, the normal pair of a
step, the first-order Gauss-Markov process and the two closed loops flown through `w + g_{i-1}`, in numpy.

The loops reuse oracle/sim.py's controllers unchanged and tests/wind_ref.py's plant step in a field; in constant wind the plant
step is oracle/sim.py's disc_dyn_glrk with the drone's own wind.  The kernels round o = a o + s xi and g = w_own o + w_form h as
one fma each, this statement as a product and a sum: they differ by an ulp per step, which the contraction a < 1 keeps from growing.
"""
import numpy as np

import wind_ref as R
from oracle import sim as S

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of integers below 2^32 (broadcast) -> (..., 4) uint64 holding the four 32-bit outputs."""
    ctr = np.asarray(ctr, dtype=np.uint64); key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).copy() for i in range(4)]
    k = [np.broadcast_to(key[..., i], shape).copy() for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]; p1 = np.uint64(M1) * c[2]             # < 2^64: exact
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1)


def normals(seed, stream, phase, part, step):
    """(xi_x, xi_y) of (seed, stream, phase, part, step); stream and step broadcast."""
    stream = np.asarray(stream, dtype=np.uint64); step = np.asarray(step, dtype=np.uint64)
    stream, step = np.broadcast_arrays(stream, step)
    seed = int(seed)
    ctr = np.stack([step, stream & MASK, stream >> np.uint64(32), np.full(stream.shape, 2 * int(phase) + int(part), dtype=np.uint64)], -1)
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    f = lambda hi, lo: ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53  # noqa: E731
    u1, u2 = f(r[..., 0], r[..., 1]), f(r[..., 2], r[..., 3])
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


class Process:
    """The gust of N drones, streams stream_base .. stream_base + N - 1: state gs (4, N) and the combination g (2, N).
    gm: a dict with seed, a, s, sigma, w_own, w_form (d2d.wind.GustModel.lower's numbers)."""

    def __init__(self, gm, N, n_ac, phase, stream_base=0, state=None, step_base=0):
        self.gm, self.phase, self.step_base = gm, int(phase), int(step_base)
        self.own = np.arange(N, dtype=np.uint64) + np.uint64(stream_base)
        self.form = self.own // np.uint64(n_ac)
        if state is None:
            self.gs = np.zeros((4, N))
            self.gs[0], self.gs[1] = (gm['sigma'] * x for x in normals(gm['seed'], self.own, phase, 0, self.step_base))
            if gm['w_form'] != 0.0:
                self.gs[2], self.gs[3] = (gm['sigma'] * x for x in normals(gm['seed'], self.form, phase, 1, self.step_base))
        else:
            self.gs = np.array(state, dtype=np.float64)

    def g(self):
        return self.gm['w_own'] * self.gs[:2] + self.gm['w_form'] * self.gs[2:]

    def advance(self, i, mask=None):
        """the draw at step i; mask (N,) bool: the drones that advance (the others are frozen)"""
        a, s = self.gm['a'], self.gm['s']
        new = self.gs.copy()
        nx, ny = normals(self.gm['seed'], self.own, self.phase, 0, self.step_base + i)
        new[0], new[1] = a * self.gs[0] + s * nx, a * self.gs[1] + s * ny
        if self.gm['w_form'] != 0.0:
            mx, my = normals(self.gm['seed'], self.form, self.phase, 1, self.step_base + i)
            new[2], new[3] = a * self.gs[2] + s * mx, a * self.gs[3] + s * my
        self.gs = new if mask is None else np.where(mask, new, self.gs)


def sample(gm, N, n_rows, n_ac, phase, stream_base=0, state=None, step_base=0):
    """d2d_gust_sample: g (n_rows, 2, N), the states after every row gs (n_rows, 4, N)."""
    pr = Process(gm, N, n_ac, phase, stream_base, state, step_base)
    g = np.zeros((n_rows, 2, N)); gs = np.zeros((n_rows, 4, N))
    g[0], gs[0] = pr.g(), pr.gs
    for i in range(1, n_rows):
        pr.advance(i)
        g[i], gs[i] = pr.g(), pr.gs
    return g, gs


def _plant(X, U, w, g, field, t, dt, tau_phi, tau_v):
    """one plant step of n drones in w + g (constant wind w) or field + g: g (2, n)"""
    if field is None:
        return S.disc_dyn_glrk(X, U, (w[0] + g[0], w[1] + g[1]), dt, tau_phi, tau_v)
    return disc_dyn_glrk_gust(X, U, field, g, t, dt, tau_phi, tau_v)


class _Offset:
    """field + a constant per drone: what a GUST panel reads (sample_many is called with the drones on the last axis)."""

    def __init__(self, field, g):
        self.field, self.g = field, g

    def sample_many(self, t, x, y):
        wx, wy = self.field.sample_many(t, x, y)
        return wx + self.g[0], wy + self.g[1]


def _panels_stacked(x, y, psi, dphi, dv, phi_c, v_c, field, t, mesh, ns):
    """wind_ref._panels_wind, statement for statement, with the ns stage evaluations of a sweep in ONE sample_many call (arrays
    (ns, n)): the closed loops call it 400 times per case."""
    c, b, A = S.gauss_tableau(ns)
    tp = t
    for row in mesh:
        w = row[0]
        vv = np.array([v_c + dv * row[1 + ns + i] for i in range(ns)])
        h = np.array([S.G_ACC * np.tan(phi_c + dphi * row[1 + i]) / vv[i] for i in range(ns)])
        ps = np.array([psi + w * sum(A[i, j] * h[j] for j in range(ns)) for i in range(ns)])
        ax, ay = vv * np.cos(ps), vv * np.sin(ps)
        w0x, w0y = field.sample_many(tp, x, y)
        ux = np.broadcast_to(w0x, ax.shape).copy(); uy = np.broadcast_to(w0y, ay.shape).copy()
        px = np.array([x + w * sum(A[i, j] * (ax[j] + ux[j]) for j in range(ns)) for i in range(ns)])
        py = np.array([y + w * sum(A[i, j] * (ay[j] + uy[j]) for j in range(ns)) for i in range(ns)])
        tx, ty = R.WIND_TOL * (1.0 + np.abs(x)), R.WIND_TOL * (1.0 + np.abs(y))
        ts = np.broadcast_to(tp, np.shape(x))[None] + (c * w)[:, None]
        for _ in range(R.WIND_MAX_ITERS):
            ux, uy = field.sample_many(ts, px, py)
            nx = np.array([x + w * sum(A[i, j] * (ax[j] + ux[j]) for j in range(ns)) for i in range(ns)])
            ny = np.array([y + w * sum(A[i, j] * (ay[j] + uy[j]) for j in range(ns)) for i in range(ns)])
            ok = ~(np.abs(nx - px) > tx).any(0) & ~(np.abs(ny - py) > ty).any(0)
            px, py = nx, ny
            if ok.all():
                break
        sx = sum(b[i] * ax[i] for i in range(ns)); sy = sum(b[i] * ay[i] for i in range(ns))
        su = sum(b[i] * ux[i] for i in range(ns)); sv = sum(b[i] * uy[i] for i in range(ns))
        x = x + w * (sx + su); y = y + w * (sy + sv)
        psi = psi + w * sum(b[i] * h[i] for i in range(ns))
        dphi = dphi * row[1 + 2 * ns]; dv = dv * row[2 + 2 * ns]
        tp = tp + w
    return x, y, psi, dphi, dv


def disc_dyn_glrk_gust(Xk, Uk, field, g, t, dt, tau_phi=0.01, tau_v=1.0):
    """wind_ref.disc_dyn_glrk_wind in field + g (g (2, n), t a scalar or (n,)) with each mesh run on the drones that take it only
    (wind_ref runs both on all and selects): the sweeps then stop on those drones' convergence, a difference at the level of the
    stopping tolerance like the one between wind_ref and the kernels.  tests/test_gust_cpu.py holds the two together."""
    Xk = np.asarray(Xk, float); Uk = np.asarray(Uk, float)
    n = Xk.shape[0]
    t = np.broadcast_to(np.asarray(t, float), (n,))
    dphi0 = Xk[:, 3] - Uk[:, 0]
    sel = (np.abs(dphi0) <= S.GL_FAST_DPHI) & (dt <= S.GL_FAST_RATIO * tau_phi)
    out = np.zeros((n, 5))
    for idx, mesh, ns in ((np.nonzero(sel)[0], S.gl_mesh(dt, tau_phi, tau_v, (0.0, 1.0), S.GL_FAST_STAGES), S.GL_FAST_STAGES),
                          (np.nonzero(~sel)[0], S.gl_mesh(dt, tau_phi, tau_v), S.GL_STAGES)):
        if len(idx) == 0:
            continue
        X, U = Xk[idx], Uk[idx]
        x, y, psi, dphi, dv = _panels_stacked(X[:, 0].copy(), X[:, 1].copy(), X[:, 2].copy(), X[:, 3] - U[:, 0], X[:, 4] - U[:, 1], U[:, 0],
                                              U[:, 1], _Offset(field, g[:, idx]), t[idx], mesh, ns)
        out[idx] = np.stack([x, y, S.norm_mpi_pi(psi), U[:, 0] + dphi, U[:, 1] + dv], axis=-1)
    return out


def formation_gvf_run_gust(c, r, v_c, X0, n_steps, dt, gm, phase, n_form=1, stream_base=0, state=None, W=(0.0, 0.0), field=None,
                           t_start=0.0, X0f=None, stop_tol=None, ke=4e-4, kd=25.0, kr=20.0, tau_phi=0.01, tau_v=1.0):
    """oracle/sim.py formation_gvf_run for n_form formations on the circles c (n_ac, 2) from X0 (n_ac, 5) or (n_form, n_ac, 5), each
    with its own gusts (drone d = formation * n_ac + aircraft draws on stream stream_base + d), the plant in W + g or field + g; the
    law sees no wind.  X0f (n_form, n_ac, >= 3), stop_tol: the state rule of case 1 per formation (`break` at the top of step i once
    every aircraft was within stop_tol of X0f after step i - 1, i - 1 > 0); a formation that has stopped is frozen, its gust too.
    Returns X (T, n_form, n_ac, 5), U (T, n_form, n_ac, 2), g (T, 2, N), stop_row (n_form,), the gust state (4, N) after each
    formation's last executed step."""
    c = np.asarray(c, float); n_ac = c.shape[0]; N = n_form * n_ac
    B = S.construct_b_matrix(n_ac); z_des = np.zeros(n_ac - 1)
    X = np.zeros((n_steps, n_form, n_ac, 5)); U = np.zeros((n_steps, n_form, n_ac, 2)); G = np.zeros((n_steps, 2, N))
    pr = Process(gm, N, n_ac, phase, stream_base, state)
    X[0] = X0; G[0] = pr.g()
    stop_row = np.full(n_form, n_steps); ok = np.zeros(n_form, bool)
    for i in range(1, n_steps):
        if X0f is not None and i - 1 > 0:
            stop_row = np.where(ok & (stop_row == n_steps), i, stop_row)
        run = stop_row == n_steps
        if not run.any():
            break
        for k in np.nonzero(run)[0]:
            U_r, _ = S.dcf_get(B, c, X[i - 1, k][:, :2].T.copy(), z_des, kr)
            Rr = U_r + r
            for j in range(n_ac):
                e, n, H = S.circle_get(X[i - 1, k, j], c[j], Rr[j])
                Ug, _, _ = S.gvf_get(X[i - 1, k, j], ke, kd, e, n, H)
                U[i - 1, k, j] = [np.arctan(Ug / 9.81), v_c]
        d = np.nonzero(np.repeat(run, n_ac))[0]                           # the drones of the running formations
        Xn = _plant(X[i - 1].reshape(N, 5)[d], U[i - 1].reshape(N, 2)[d], W, pr.g()[:, d], field, t_start + (i - 1) * dt, dt, tau_phi, tau_v)
        X[i] = X[i - 1]
        X[i].reshape(N, 5)[d] = Xn
        pr.advance(i, np.repeat(run, n_ac))
        G[i] = pr.g()
        if X0f is not None:
            ok = (np.abs(X[i][:, :, :3] - np.asarray(X0f)[:, :, :3]) <= np.asarray(stop_tol)).all((1, 2))
    return X, U, G, stop_row, pr.gs


def track_run_gust(time, x_ref, y_ref, X0s, w, gm, phase, n_ac=1, stream_base=0, state=None, field=None, t_start=None,
                   tau_phi=0.01, tau_v=1.0):
    """oracle/sim.py track_run with the plant in w + g or field + g (drone j's step i from t_start[j] + (i - 1) dt; None: time[0]);
    the controller keeps the constant w.  Returns X, U, Xr (T, n, .), g (T, 2, n), the final gust state."""
    T, n = x_ref.shape
    dt = time[1] - time[0]
    t0 = np.full(n, time[0]) if t_start is None else np.asarray(t_start, float)
    X = np.zeros((T, n, 5)); U = np.zeros((T, n, 2)); Xr = np.zeros((T, n, 5)); G = np.zeros((T, 2, n))
    F = [S.compute_derivatives(x_ref[:, j], y_ref[:, j], dt) for j in range(n)]
    pr = Process(gm, n, n_ac, phase, stream_base, state)
    X[0] = np.asarray(X0s, float); G[0] = pr.g()
    for i in range(1, T):
        for j in range(n):
            Fdx, Fdy, Fddx, Fddy = F[j]
            Xr[i - 1, j], _, U[i - 1, j], _ = S.compute_gain(X[i - 1, j], [x_ref[i, j], y_ref[i, j]], [Fdx[i], Fdy[i]],
                                                             [Fddx[i], Fddy[i]], [0, 0], w, tau_phi, tau_v)
        X[i] = _plant(X[i - 1], U[i - 1], w, pr.g(), field, t0 + (i - 1) * dt, dt, tau_phi, tau_v)
        pr.advance(i)
        G[i] = pr.g()
    return X, U, Xr, G, pr.gs
