"""Inputs and oracle answers of the single-evaluation entry points (include/d2d.h: d2d_flatness, d2d_cont_jac, d2d_gvf_eval,
d2d_dcf_eval, d2d_lqr) and of the fit helpers (d2d_fit_project / _coeffs / _sample), at the ragged sizes where a planar [c][n] kernel
goes wrong.  CPU only: every answer is computed element by element by oracle/sim.py and oracle/fit.py, nothing is restated here.
tests/test_helper_cases_cpu.py asserts what this file claims; tests/test_gpu_helpers.py compares the kernels with it.

Every array is planar as the C ABI takes it: component-major, the batch index last."""
import numpy as np

from oracle import fit as F, sim as S

NS = (1, 63, 64, 65, 255, 256, 257, 513)            # the 256-thread kernels: wave and block edges, three blocks
NS_LQR = (1, 63, 64, 65, 129)                       # 64-thread blocks whose dead lanes are clamped to n - 1
N_FORMS = (1, 255, 256, 257)
N_ACS = (1, 2, 4, 5, 64)                            # incidence matrix; a dense random B for DENSE_N_ACS
DENSE_N_ACS = (3, 5)
FIT_BS = (1, 3, 4, 5, 37)                           # fit_project / fit_init: four trajectories per block

V_AIR = (6.0, 20.0)                                 # airspeed |Yd - w| [m/s]
PHI_ABS = 0.95                                      # |phi| < 1 rad
GVF_MIN_DIST = 1.0                                  # GVF points at least 1 m off the circle's centre
NEAR_PI = 1e-9                                      # a random formation with an unwrapped error this near +-pi is dropped
# per size index: (wind, tau_phi, tau_v); the odd ones have wind and lags away from the defaults
_PLANT = (((0.0, 0.0), 0.01, 1.0), ((1.5, -0.7), 0.05, 0.8), ((0.0, 0.0), 0.01, 1.0), ((-2.0, 1.1), 0.2, 1.7),
          ((0.0, 0.0), 0.01, 1.0), ((0.6, 2.4), 0.0333, 0.5), ((0.0, 0.0), 0.01, 1.0), ((-1.2, -1.9), 0.11, 2.5))
_GVF_GAINS = ((4e-4, 25.0), (1e-3, 10.0), (4e-4, 25.0), (2.5e-4, 40.0), (4e-4, 25.0), (7e-4, 18.0), (4e-4, 25.0), (5e-5, 33.0))


def _rng(*key):
    return np.random.default_rng([20250611, *key])


def probe_indices(n):
    """At least 8 indices of a batch of n (all of it when n < 8): both ends and both sides of every 64 and 256 boundary."""
    idx = {0, n - 1} | {b + d for b in range(64, n + 1, 64) for d in (-1, 0)} | set(range(min(n, 8)))
    return sorted(i for i in idx if 0 <= i < n)


# ---- flatness maps ------------------------------------------------------------------------------------------------------------
def flatness_case(variant, n):
    """d2d_flatness: Yref [8][n] = (Y, Yd, Ydd, Yddd) x (x, y) -> X [5][n], U [2][n], Xdot [5][n] (variant 0 only)."""
    (wx, wy), tau_phi, tau_v = _PLANT[NS.index(n)]
    r = _rng(1, variant, n)
    va, psi = r.uniform(V_AIR[0] + 0.1, V_AIR[1] - 0.1, n), r.uniform(-np.pi, np.pi, n)
    phi = r.uniform(-PHI_ABS, PHI_ABS, n)
    along = r.uniform(-2.0, 2.0, n)
    lat = S.G_ACC * np.tan(phi)                                  # the lateral acceleration that banks by phi
    ux, uy = np.cos(psi), np.sin(psi)
    Yref = np.empty((8, n))
    Yref[0:2] = r.uniform(-150.0, 150.0, (2, n))
    Yref[2], Yref[3] = va * ux + wx, va * uy + wy
    Yref[4], Yref[5] = along * ux - lat * uy, along * uy + lat * ux
    Yref[6:8] = r.uniform(-1.5, 1.5, (2, n))
    X, U, Xdot = np.zeros((5, n)), np.zeros((2, n)), np.zeros((5, n))
    for i in range(n):
        Ys = Yref[:, i].reshape(4, 2)
        if variant == 0:
            X[:, i], U[:, i], Xdot[:, i] = S.flat_state_input(Ys, (wx, wy), tau_phi, tau_v)
        else:
            X[:, i], U[:, i] = S.compute_flatness(Ys[0], Ys[1], Ys[2], Ys[3], (wx, wy), tau_phi, tau_v)
    return dict(variant=variant, n=n, w=(wx, wy), tau_phi=tau_phi, tau_v=tau_v, Yref=Yref, X=X, U=U, Xdot=Xdot)


def cont_jac_case(n):
    """d2d_cont_jac: Xr [5][n] -> A [25][n] (row-major 5x5), B [10][n] (row-major 5x2)."""
    _, tau_phi, tau_v = _PLANT[NS.index(n)]
    r = _rng(2, n)
    Xr = np.stack([r.uniform(-150, 150, n), r.uniform(-150, 150, n), r.uniform(-np.pi, np.pi, n),
                   r.uniform(-PHI_ABS, PHI_ABS, n), r.uniform(*V_AIR, n)])
    A, B = np.empty((25, n)), np.empty((10, n))
    for i in range(n):
        Ai, Bi = S.cont_jac(Xr[:, i], tau_phi, tau_v)
        A[:, i], B[:, i] = Ai.reshape(25), np.asarray(Bi, float).reshape(10)
    return dict(n=n, tau_phi=tau_phi, tau_v=tau_v, Xr=Xr, A=A, B=B)


# ---- guidance vector field ------------------------------------------------------------------------------------------------------
def gvf_case(n):
    """d2d_gvf_eval: X [5][n], e [n], nvec [2][n], H [4][n] (CircleTraj.get of each point) -> U [3][n] = U, U1, U2."""
    ke, kd = _GVF_GAINS[NS.index(n)]
    r = _rng(3, n)
    c = r.uniform(-80.0, 80.0, (2, n))
    dist, ang = r.uniform(GVF_MIN_DIST, 140.0, n), r.uniform(-np.pi, np.pi, n)
    radius = r.uniform(20.0, 90.0, n)
    X = np.stack([c[0] + dist * np.cos(ang), c[1] + dist * np.sin(ang), r.uniform(-np.pi, np.pi, n),
                  r.uniform(-PHI_ABS, PHI_ABS, n), r.uniform(*V_AIR, n)])
    e, nvec, H, U = np.empty(n), np.empty((2, n)), np.empty((4, n)), np.empty((3, n))
    for i in range(n):
        ei, ni, Hi = S.circle_get(X[:, i], c[:, i], radius[i])
        e[i], nvec[:, i], H[:, i] = ei, ni, Hi.reshape(4)
        U[:, i] = S.gvf_get(X[:, i], ke, kd, ei, ni, Hi)
    return dict(n=n, ke=ke, kd=kd, c=c, radius=radius, X=X, e=e, nvec=nvec, H=H, U=U)


# ---- formation phase control ----------------------------------------------------------------------------------------------------
EDGE_UNWRAPPED = (np.pi, -np.pi, 2 * np.pi)          # what the oracle turns into pi, pi, 0
_EDGE_THETA = ((0.0, np.pi), (np.pi, 0.0), (-np.pi, np.pi))          # phases of aircraft 0 and 1 with those differences
_EDGE_OFFSET = {0.0: (1.0, 0.0), np.pi: (-1.0, 0.0), -np.pi: (-1.0, -0.0)}    # atan2(+-0.0, -1) = +-pi exactly


def unwrapped_error(B, c, p, z_des):
    """B^T theta - z_des of one formation before DCFController.get wraps it (the first three lines of oracle/sim.py dcf_get)."""
    pos = p - c.T
    return B.T @ np.arctan2(pos[1], pos[0]) - z_des


def edge_formation(kind, n_ac):
    """(c (n_ac, 2), p (2, n_ac)) of a formation whose first unwrapped error is exactly EDGE_UNWRAPPED[kind] under the incidence
    matrix with z_des = 0: every aircraft sits at (+-1, +-0.0) from a centre with integer x and y = +0.0, so every phase is one of
    0, pi, -pi and every difference of neighbours is exact.  The aircraft behind the first two repeat the phase of aircraft 1."""
    th = list(_EDGE_THETA[kind]) + [_EDGE_THETA[kind][1]] * (n_ac - 2)
    c = np.zeros((n_ac, 2)); c[:, 0] = 7.0 * np.arange(n_ac) - 3.0
    off = np.array([_EDGE_OFFSET[t] for t in th[:n_ac]])
    return c, np.stack([c[:, 0] + off[:, 0], off[:, 1]])          # (y itself is the offset: 0.0 + -0.0 would lose the sign)


def dcf_case(n_form, n_ac, dense=False):
    """d2d_dcf_eval: centres, pos [2][N] (N = n_form n_ac, aircraft a of formation f at f n_ac + a), host B (n_ac, n_ac - 1) and
    z_des -> U_r [N], eth_deg [n_form (n_ac - 1)].  dense: B ~ N(0, 2) instead of the incidence matrix, z_des random.
    Incidence cases of more than one formation and more than one aircraft carry the three edge formations (z_des = 0 then) at
    'edges' = [(formation, kind)]; random formations within NEAR_PI of a wrap threshold are dropped ('dropped' of 'drawn')."""
    r = _rng(4, n_form, n_ac, int(dense))
    nm = n_ac - 1
    if dense:
        B = r.normal(0.0, 2.0, (n_ac, nm)); z_des = r.uniform(-np.pi, np.pi, nm)
    else:
        B = S.construct_b_matrix(n_ac); z_des = np.zeros(nm)
    kr = 20.0 if (n_form + n_ac) % 2 else 7.5
    edges = [] if (dense or n_ac < 2 or n_form < 3) else [(1, 0), (n_form // 2, 1), (n_form - 2, 2)]
    at = dict(edges)
    cs, ps, raws = [], [], []
    drawn = dropped = 0
    for f in range(n_form):
        if f in at:
            c, p = edge_formation(at[f], n_ac)
        else:
            while True:
                c = r.uniform(-100.0, 100.0, (n_ac, 2))
                d, a = r.uniform(1.0, 90.0, n_ac), r.uniform(-np.pi, np.pi, n_ac)
                p = (c + np.stack([d * np.cos(a), d * np.sin(a)], 1)).T.copy()
                drawn += 1
                raw = unwrapped_error(B, c, p, z_des)
                if nm == 0 or np.abs(np.abs(raw) - np.pi).min() > NEAR_PI:
                    break
                dropped += 1
        cs.append(c); ps.append(p); raws.append(unwrapped_error(B, c, p, z_des))
    U_r, eth = np.empty((n_form, n_ac)), np.empty((n_form, nm))
    for f in range(n_form):
        U_r[f], e = S.dcf_get(B, cs[f], ps[f], z_des, kr)
        eth[f] = np.rad2deg(e)
    centres = np.concatenate(cs).T.copy()                       # [2][N]
    pos = np.concatenate(ps, axis=1)
    return dict(n_form=n_form, n_ac=n_ac, dense=dense, B=B, z_des=z_des, kr=kr, centres=centres, pos=pos, U_r=U_r.reshape(-1),
                eth_deg=eth.reshape(-1), raw=np.array(raws), edges=edges, drawn=drawn, dropped=dropped)


def dcf_cases():
    return [dcf_case(nf, na) for na in N_ACS for nf in N_FORMS] + [dcf_case(nf, na, True) for na in DENSE_N_ACS for nf in N_FORMS]


# ---- LQR --------------------------------------------------------------------------------------------------------------------------
LQR_R = np.array([[2.0, 0.3], [0.3, 1.0]])


def lqr_case(n):
    """d2d_lqr on random 5-state / 2-input systems (the distribution of tests/test_gpu_mirror.py test_lqr_vs_scipy_care):
    A [25][n], B [10][n], host Q (5, 5), R (2, 2) -> K [10][n], P [25][n]."""
    r = _rng(5, n)
    A, Bm = r.normal(0, 1.0, (n, 5, 5)), r.normal(0, 1.0, (n, 5, 2))
    Qh = r.normal(0, 1, (5, 5)); Q = Qh @ Qh.T + 0.1 * np.eye(5)
    K, P = np.empty((n, 2, 5)), np.empty((n, 5, 5))
    for i in range(n):
        K[i], P[i] = S.lqr(A[i], Bm[i], Q, LQR_R)
    pl = lambda M: np.ascontiguousarray(M.reshape(n, -1).T)          # noqa: E731
    return dict(n=n, Q=Q, R=LQR_R, A=pl(A), B=pl(Bm), K=pl(K), P=pl(P))


# ---- fit helpers ------------------------------------------------------------------------------------------------------------------
def fit_scenarios(B, K, seed):
    """B scenario rows of a K-node plan; every other row flies in a wind."""
    sc = F.set_scale(F.synth_scenarios(B, seed=seed), 0.1, K)
    r = _rng(6, B, K, seed)
    sc[1::2, F.SC_WX], sc[1::2, F.SC_WY] = r.uniform(-2.5, 2.5, (2, len(sc[1::2])))
    if B == 1:
        sc[0, F.SC_WX], sc[0, F.SC_WY] = 1.5, -0.7
    return sc


def fit_case(basis, B, seed=7):
    """Inputs and oracle answers of the three helpers for a plan whose oracle basis is `basis` (F.FitBasis.from_arrays of the plan's
    own arrays): scen (B, 80); xy (B, 2, K) random node positions with q_xy = F.initial_guess(basis, sc, wp=xy); wp (B, 2, K) the
    oracle's 'tri' waypoints with q_wp their projection; then at q = q_wp + noise: z (B, 2, S, 8), Y (B, 6, K), Xs (B, 5, K)."""
    K, n = basis.K, 2 * basis.nq
    sc = fit_scenarios(B, K, seed)
    r = _rng(7, B, K, basis.S)
    wp = np.array([np.stack(F.waypoints(sc[i], K, basis.duration)) for i in range(B)])
    xy = wp + r.normal(0.0, 2.0, wp.shape)
    q_xy = np.array([F.initial_guess(basis, sc[i], wp=(xy[i, 0], xy[i, 1])) for i in range(B)])
    q_wp = np.array([F.initial_guess(basis, sc[i], wp=(wp[i, 0], wp[i, 1])) for i in range(B)])
    q = q_wp + r.normal(0.0, 0.05, (B, n))
    z, Y, Xs = np.empty((B, 2, basis.S, 8)), np.empty((B, 6, K)), np.empty((B, 5, K))
    for i in range(B):
        z[i] = F.coefficients(basis, sc[i], q[i])
        Yo = F.flat_outputs(basis, sc[i], q[i])                  # (3, 2, K)
        Y[i] = Yo.reshape(6, K)
        va, psi, phi = F.flatness(Yo, sc[i])
        Xs[i] = np.stack([Yo[0, 0], Yo[0, 1], psi, phi, va])
    return dict(B=B, scen=sc, xy=xy, wp=wp, q_xy=q_xy, q_wp=q_wp, q=q, z=z, Y=Y, Xs=Xs)


def fit_lattice_case(basis, B):
    """Scenario rows whose 'tri' waypoints are integers on both legs: the end points lie 2 (n1 - 1) (n2 - 1) k apart on each axis
    (n1 = K // 2, n2 = K - n1 nodes per leg), farther than vref x duration, so the dog-leg's apex is the midpoint and every
    np.linspace step is an integer.  Such waypoints come out the same from any correct evaluation order, fused multiply-adds
    included: the oracle's are, bit for bit, the ones d2d_fit_init forms on the device."""
    K = basis.K
    n1 = K // 2; n2 = K - n1
    L = 2.0 * (n1 - 1) * (n2 - 1)
    sc = fit_scenarios(B, K, 11)
    for i in range(B):
        kx, ky = ((1, -1), (-1, 2), (2, 1), (1, 3), (-3, -2))[i % 5]         # (never 0: np.linspace then divides before it multiplies)
        sc[i, F.SC_X0], sc[i, F.SC_Y0] = float(3 * i - 40), float(17 - 5 * i)
        sc[i, F.SC_X1], sc[i, F.SC_Y1] = sc[i, F.SC_X0] + kx * L, sc[i, F.SC_Y0] + ky * L
    wp = np.array([np.stack(F.waypoints(sc[i], K, basis.duration)) for i in range(B)])
    q = np.array([F.initial_guess(basis, sc[i], wp=(wp[i, 0], wp[i, 1])) for i in range(B)])
    return dict(B=B, scen=sc, wp=wp, q_wp=q)
