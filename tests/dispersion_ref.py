"""CPU statement of d2d_track_dispersion (include/d2d.h, version 128): the covariance of the deviation of the gust flight of the
tracking loop from its gust-free flight, propagated row by row.  numpy and scipy only.

Deviation state of one drone z = (dx, dy, dpsi, dphi, dv, gx, gy); S its 7 x 7 covariance.
  S_0 = blockdiag(P0 or 0_5, sigma^2 I_2)
  step i = 1 .. T - 1 with reference sample i:  Xr_i, K_i = ComputeGain at X = Xr_i (oracle/sim.py compute_gain: quirky cont_jac, CARE,
  Yddd = 0);  A_i = the TRUE Jacobian of oracle/sim.py cont_dyn at Xr_i;  [Ad Bd Ed] = rows 0..4 of expm(dt [[A B E], [0 0 0]]);
  F_i = [[Ad - Bd K_i, Ed], [0, a I_2]];  S_i = F_i S_{i-1} F_i^T + diag(0_5, s^2, s^2).
Saturations and the psi wrap are ignored.  `dispersion_ld` is an independent second evaluation (np.longdouble, the exponential by a plain
scaled Taylor series): the difference between the two is the floor of every comparison against this file."""
import ctypes as C

import numpy as np
import scipy.linalg

from oracle import sim as S

NS = 7
TRI = [(i, j) for i in range(NS) for j in range(i + 1)]          # packed lower triangle: (i, j), i >= j, at i (i + 1) / 2 + j


def pack(Sm):
    return np.array([Sm[i, j] for i, j in TRI])


def unpack(v):
    Sm = np.zeros((NS, NS), dtype=np.asarray(v).dtype)
    for q, (i, j) in enumerate(TRI):
        Sm[i, j] = Sm[j, i] = v[q]
    return Sm


def derivatives(x_ref, y_ref, dt):
    """The tracking loop's derivatives (oracle/sim.py compute_derivatives) of one drone's reference; two rows have no second-order edge
    formula: the one first difference on both rows (numpy.gradient's edge_order=1), hence a zero second derivative."""
    eo = 2 if len(x_ref) >= 3 else 1
    g = lambda f: np.gradient(f, edge_order=eo) / dt            # noqa: E731
    Fdx, Fdy = g(np.asarray(x_ref, float)), g(np.asarray(y_ref, float))
    return Fdx, Fdy, g(Fdx), g(Fdy)


def plant_jac(Xr, tau_phi=0.01, tau_v=1.0, quirk=False):
    """A = d f / d X of cont_dyn at (psi, phi, v) = Xr[2:5], B = d f / d U, E = d f / d W.  quirk: cont_jac's row 2 instead (a variant
    for the tests' power check: that row belongs to the controller, not to the plant)."""
    A, B = S.cont_jac(Xr, tau_phi, tau_v)
    if not quirk:
        phi, v = Xr[3], Xr[4]
        A[2, 3] = S.G_ACC / (v * np.cos(phi) ** 2)
        A[2, 4] = -S.G_ACC * np.tan(phi) / v ** 2
    E = np.zeros((5, 2)); E[0, 0] = E[1, 1] = 1.0
    return A, B.astype(float), E


def zoh(A, B, E, dt):
    M = np.zeros((9, 9))
    M[:5, :5], M[:5, 5:7], M[:5, 7:9] = A, B, E
    X = scipy.linalg.expm(dt * M)
    return X[:5, :5], X[:5, 5:7], X[:5, 7:9]


def zoh_ld(A, B, E, dt):
    """The same in np.longdouble by scaling and squaring of a plain Taylor series."""
    ld = np.longdouble
    M = np.zeros((9, 9), dtype=ld)
    M[:5, :5], M[:5, 5:7], M[:5, 7:9] = A, B, E
    M = M * ld(dt)
    sq = max(0, int(np.ceil(np.log2(max(float(np.abs(M).sum(1).max()), 1e-300)))) + 4)      # |M| / 2^sq <= 1 / 16
    M = M / ld(2.0) ** sq
    X, term = np.eye(9, dtype=ld), np.eye(9, dtype=ld)
    for k in range(1, 25):
        term = term @ M / ld(k)
        X = X + term
    for _ in range(sq):
        X = X @ X
    return X[:5, :5], X[:5, 5:7], X[:5, 7:9]


def reference_gains(x_ref, y_ref, dt, w=(0.0, 0.0), tau_phi=0.01, tau_v=1.0, deriv=None, **gain_kw):
    """Xr (T, 5) and K (T, 2, 5) of rows 1 .. T - 1 of one drone (row 0 is not used: zeros).  deriv: (Fdx, Fdy, Fddx, Fddy), each (T,),
    to use instead of derivatives()."""
    T = len(x_ref)
    Fdx, Fdy, Fddx, Fddy = derivatives(x_ref, y_ref, dt) if deriv is None else deriv
    Xr, K = np.zeros((T, 5)), np.zeros((T, 2, 5))
    for i in range(1, T):
        Xr[i], _, _, K[i] = S.compute_gain(np.zeros(5), [x_ref[i], y_ref[i]], [Fdx[i], Fdy[i]], [Fddx[i], Fddy[i]], [0, 0], w, tau_phi, tau_v,
                                           **gain_kw)
    return Xr, K


def reference_states(x_ref, y_ref, dt, w=(0.0, 0.0), tau_phi=0.01, tau_v=1.0, deriv=None):
    """Xr (T, 5) alone (no Riccati solve): for callers that bring K."""
    T = len(x_ref)
    Fdx, Fdy, Fddx, Fddy = derivatives(x_ref, y_ref, dt) if deriv is None else deriv
    Xr = np.zeros((T, 5))
    for i in range(1, T):
        Xr[i], _ = S.compute_flatness([x_ref[i], y_ref[i]], [Fdx[i], Fdy[i]], [Fddx[i], Fddy[i]], [0, 0], w, tau_phi, tau_v)
    return Xr


def _lam_max(xx, xy, yy):
    hd = 0.5 * (xx - yy)
    return 0.5 * (xx + yy) + np.sqrt(hd * hd + xy * xy)


def dispersion(x_ref, y_ref, dt, a, s, sigma, w=(0.0, 0.0), tau_phi=0.01, tau_v=1.0, S0=None, K=None, edges=None, discs=None,
               quirk=False, no_gust_input=False, longdouble=False, deriv=None, **gain_kw):
    """One drone.  x_ref, y_ref (T,); a, s, sigma: the gust's numbers (d2d.wind.GustModel.numbers(dt)); S0: packed (28,) or None;
    K (T, 2, 5): the gains to use (rows 1 ..), None: oracle/sim.py compute_gain's; edges (k, 4), discs (k, 3): the rows of d2d_fence and
    d2d_keep_out for this drone.  quirk, no_gust_input (Ed = 0): variants for the tests' power check.
    deriv: the reference's derivatives (Fdx, Fdy, Fddx, Fddy), each (T,), None: derivatives().  Differentiating twice amplifies the
    rounding of the first pass (by ~ v / (a dt)), and on the edge rows a device may contract the three-term formula: a GPU test
    hands over the values the tracking loop itself recorded (Yd_hist, Ydd_hist), as it hands over K.
    Returns dict(Ppos (T, 3) = xx, xy, yy; S packed (28,); S_hist (T, 28); sig_max, sig_row; fence_sn, fence_k, fence_row (k,);
    disc_k, disc_row (k,)), and what the extremes were taken over, entry q for row q + 1: sig_rows (T - 1,), fence_sn_rows,
    fence_k_rows, disc_sn_rows, disc_k_rows (k, T - 1)."""
    ft = np.longdouble if longdouble else np.float64
    x_ref, y_ref = np.asarray(x_ref, float), np.asarray(y_ref, float)
    T = len(x_ref)
    if K is None:
        Xr, K = reference_gains(x_ref, y_ref, dt, w, tau_phi, tau_v, deriv, **gain_kw)
    else:
        Xr = reference_states(x_ref, y_ref, dt, w, tau_phi, tau_v, deriv)
    Sm = np.zeros((NS, NS), dtype=ft)
    if S0 is None:
        Sm[5, 5] = Sm[6, 6] = ft(sigma) ** 2
    else:
        Sm = unpack(np.asarray(S0)).astype(ft)
    Qn = np.zeros((NS, NS), dtype=ft); Qn[5, 5] = Qn[6, 6] = ft(s) ** 2
    hist = np.zeros((T, 28), dtype=ft)
    hist[0] = pack(Sm)
    for i in range(1, T):
        A, B, E = plant_jac(Xr[i], tau_phi, tau_v, quirk)
        Ad, Bd, Ed = (zoh_ld if longdouble else zoh)(A, B, E, dt)
        F = np.zeros((NS, NS), dtype=ft)
        F[:5, :5] = Ad - Bd @ np.asarray(K[i]).astype(ft)
        if not no_gust_input:
            F[:5, 5:] = Ed
        F[5, 5] = F[6, 6] = ft(a)
        Sm = F @ Sm @ F.T + Qn
        Sm = 0.5 * (Sm + Sm.T)
        hist[i] = pack(Sm)
    out = dict(S=hist[-1].copy(), S_hist=hist, Ppos=hist[:, [0, 1, 2]].copy())
    xx, xy, yy = (hist[1:, q].astype(float) for q in (0, 1, 2))
    sg = np.sqrt(np.maximum(_lam_max(xx, xy, yy), 0.0))
    out['sig_max'], out['sig_row'], out['sig_rows'] = float(sg.max()), 1 + int(np.argmax(sg)), sg
    px, py = x_ref[1:], y_ref[1:]
    with np.errstate(divide='ignore', invalid='ignore'):
        if edges is not None:
            edges = np.asarray(edges, float)
            sn_, k_, r_, snr, kr = [], [], [], [], []
            for ex, ey, b, _ in edges:
                if ex == 0.0 and ey == 0.0:
                    sn_.append(0.0); k_.append(np.inf); r_.append(-1); snr.append(0.0 * xx); kr.append(np.inf + 0.0 * xx)
                    continue
                sn = np.sqrt(np.maximum(ex * ex * xx + 2 * ex * ey * xy + ey * ey * yy, 0.0))
                k = np.where(sn > 0, (b - (ex * px + ey * py)) / sn, np.inf)
                sn_.append(float(sn.max())); k_.append(float(k.min())); r_.append(1 + int(np.argmin(k))); snr.append(sn); kr.append(k)
            out['fence_sn'], out['fence_k'], out['fence_row'] = np.array(sn_), np.array(k_), np.array(r_, dtype=np.int32)
            out['fence_sn_rows'], out['fence_k_rows'] = np.array(snr), np.array(kr)
        if discs is not None:
            k_, r_, snr, kr = [], [], [], []
            for cx, cy, R in np.asarray(discs, float):
                if not R > 0.0:
                    k_.append(np.inf); r_.append(-1); snr.append(0.0 * xx); kr.append(np.inf + 0.0 * xx)
                    continue
                rx, ry = px - cx, py - cy
                dist = np.hypot(rx, ry)
                ux, uy = rx / dist, ry / dist
                sn = np.sqrt(np.maximum(ux * ux * xx + 2 * ux * uy * xy + uy * uy * yy, 0.0))
                k = np.where(sn > 0, (dist - R) / sn, np.inf)
                k_.append(float(k.min())); r_.append(1 + int(np.argmin(k))); snr.append(sn); kr.append(k)
            out['disc_k'], out['disc_row'] = np.array(k_), np.array(r_, dtype=np.int32)
            out['disc_sn_rows'], out['disc_k_rows'] = np.array(snr), np.array(kr)
    return out


def dispersion_ld(*args, **kw):
    """The second evaluation: every product in np.longdouble, the exponential by zoh_ld."""
    return dispersion(*args, longdouble=True, **kw)


def dispersion_batch(x_ref, y_ref, dt, a, s, sigma, S0=None, K=None, edges=None, discs=None, deriv=None, **kw):
    """n drones: x_ref, y_ref (T, n); S0 (28, n); K (T, n, 2, 5); edges (n, k, 4); discs (n, k, 3); deriv (4, T, n).  Returns a list of
    dispersion()'s dicts."""
    n = x_ref.shape[1]
    return [dispersion(x_ref[:, d], y_ref[:, d], dt, a, s, sigma, S0=None if S0 is None else S0[:, d], K=None if K is None else K[:, d],
                       edges=None if edges is None else edges[d], discs=None if discs is None else discs[d],
                       deriv=None if deriv is None else tuple(deriv[:, :, d]), **kw) for d in range(n)]


# ---- references the tests share -------------------------------------------------------------------------------------------------
def heading_speed_path(t, psi, v, p0=(0.0, 0.0), sub=16):
    """Ground positions at the times t of a path given by its heading psi(t) and ground speed v(t): Simpson-free, plain trapezoid
    on `sub` sub-intervals per step (the result only has to be a smooth reference, not the exact integral)."""
    tf = np.linspace(t[0], t[-1], (len(t) - 1) * sub + 1)
    vx, vy = v(tf) * np.cos(psi(tf)), v(tf) * np.sin(psi(tf))
    h = tf[1] - tf[0]
    x = np.concatenate([[0.0], np.cumsum(0.5 * h * (vx[1:] + vx[:-1]))])[::sub] + p0[0]
    y = np.concatenate([[0.0], np.cumsum(0.5 * h * (vy[1:] + vy[:-1]))])[::sub] + p0[1]
    return x, y


def s_turn(t, v0=15.0, amp=0.6, period=12.0, dv=0.0, theta=0.0, p0=(0.0, 0.0)):
    """An S-turn: heading theta + amp sin(2 pi t / period), speed v0 + dv t / t_end."""
    te = t[-1] - t[0]
    return heading_speed_path(t, lambda u: theta + amp * np.sin(2 * np.pi * (u - t[0]) / period), lambda u: v0 + dv * (u - t[0]) / te, p0)


def references(n, T, dt, seed=7):
    """n references of T rows, all different: drone d is straight (d % 3 == 0), a constant-rate turn (1) or an S-turn with a speed
    change (2), with its own start, heading, speed and rate.  Returns x_ref, y_ref (T, n)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    x, y = np.zeros((T, n)), np.zeros((T, n))
    for d in range(n):
        p0 = rng.uniform(-50, 50, 2)
        th, v = rng.uniform(-np.pi, np.pi), rng.uniform(11.0, 16.0)
        if d % 3 == 0:
            x[:, d], y[:, d] = p0[0] + v * np.cos(th) * t, p0[1] + v * np.sin(th) * t
        elif d % 3 == 1:
            om = rng.choice([-1.0, 1.0]) * rng.uniform(0.08, 0.3)
            x[:, d] = p0[0] + v / om * (np.sin(th + om * t) - np.sin(th))
            y[:, d] = p0[1] - v / om * (np.cos(th + om * t) - np.cos(th))
        else:
            x[:, d], y[:, d] = s_turn(t, v, rng.uniform(0.2, 0.5), max(4.0, 1.5 * T * dt), rng.uniform(-2.0, 2.0), th, p0)
    return x, y


def rel_err(got, ref_hist):
    """max over rows and entries of |got - ref| relative to the largest diagonal entry of the reference S at that row; got, ref_hist
    (T, 28) packed."""
    ref_hist = np.asarray(ref_hist, float)
    diag = np.abs(ref_hist[:, [i * (i + 1) // 2 + i for i in range(NS)]]).max(1)
    return float((np.abs(np.asarray(got, float) - ref_hist).max(1) / diag).max())


# The largest relative difference (rel_err) between dispersion and dispersion_ld over the cases of tests/test_dispersion_cpu.py,
# rounded up: what the fp64 evaluation of the statement itself is uncertain by (scipy's expm of a matrix of norm ~10 and a 7 x 7
# congruence per row).  tests/test_dispersion_cpu.py holds the measured value below it; the GPU tolerance is ten times this number.
CPU_FLOOR = 3e-15


# ---- the refusals of the entry point, for the CPU and the GPU test --------------------------------------------------------------
def entry_point_call(lib, ctx, p, x, y, din, fence, keep, dout):
    ref = lambda o: None if o is None else C.byref(o)      # noqa: E731
    return lib.d2d_track_dispersion(ctx, ref(p), x, y, ref(din), ref(fence), ref(keep), ref(dout))


def entry_point_refusals(lib, ctx, ptr):
    """Every D2D_EINVAL cause of d2d_track_dispersion -> the list of (cause, return code).  ctx: a context handle; ptr: any non-NULL
    address for the array arguments (nothing is read before the checks).  """
    import d2dhip
    P = lambda n=4, T=5: d2dhip.Context.track_params(n, T, 0.05)      # noqa: E731
    I = lambda a=0.9, s=0.1, sg=0.3: d2dhip.DispersionIn(a, s, sg, None)      # noqa: E731
    O = lambda **kw: d2dhip.DispersionOut(**kw)      # noqa: E731
    fence = lambda k=2, e=ptr: d2dhip.FenceC(k, 0, e)      # noqa: E731
    keep = lambda k=2, e=ptr: d2dhip.KeepOutC(k, 0, e)      # noqa: E731
    nan, inf = float('nan'), float('inf')
    cases = [('null in', (P(), ptr, ptr, None, None, None, O())), ('null out', (P(), ptr, ptr, I(), None, None, None)),
             ('null p', (None, ptr, ptr, I(), None, None, O())), ('null x_ref', (P(), None, ptr, I(), None, None, O())),
             ('n < 1', (P(0), ptr, ptr, I(), None, None, O())), ('n_rows < 2', (P(4, 1), ptr, ptr, I(), None, None, O())),
             ('a < 0', (P(), ptr, ptr, I(a=-0.1), None, None, O())), ('a = 1', (P(), ptr, ptr, I(a=1.0), None, None, O())),
             ('a nan', (P(), ptr, ptr, I(a=nan), None, None, O())),
             ('s < 0', (P(), ptr, ptr, I(s=-1.0), None, None, O())), ('s inf', (P(), ptr, ptr, I(s=inf), None, None, O())),
             ('sigma < 0', (P(), ptr, ptr, I(sg=-1.0), None, None, O())), ('sigma nan', (P(), ptr, ptr, I(sg=nan), None, None, O())),
             ('n_edge > max', (P(), ptr, ptr, I(), fence(d2dhip.MAX_FENCE + 1), None, O())),
             ('n_keep > max', (P(), ptr, ptr, I(), None, keep(d2dhip.MAX_KEEP + 1), O())),
             ('n_edge < 0', (P(), ptr, ptr, I(), fence(-1), None, O())),
             ('edges null', (P(), ptr, ptr, I(), fence(2, None), None, O())), ('discs null', (P(), ptr, ptr, I(), None, keep(2, None), O())),
             ('fence_sn without a fence', (P(), ptr, ptr, I(), None, None, O(fence_sn=ptr))),
             ('fence_k without edges', (P(), ptr, ptr, I(), fence(0, None), None, O(fence_k=ptr, fence_row=ptr))),
             ('disc_k without discs', (P(), ptr, ptr, I(), None, None, O(disc_k=ptr, disc_row=ptr))),
             ('fence_k without fence_row', (P(), ptr, ptr, I(), fence(), None, O(fence_k=ptr))),
             ('disc_row without disc_k', (P(), ptr, ptr, I(), None, keep(), O(disc_row=ptr)))]
    return [(name, entry_point_call(lib, ctx, *args)) for name, args in cases]
