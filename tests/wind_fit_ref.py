"""CPU statement of d2d_wind_fit (include/d2d.h; drone-sim-python_amd/csrc/wind_fit.hip) in numpy / scipy.sparse.

  sincos(psi)                      cos and sin by the header's fixed sequence of IEEE operations (no fused multiply-add)
  measure(X, n_ac, dt_row, grid..) the samples of a history: values, midpoints, rejections by reason, cells and axis weights
  design(ms, grid)                 the sparse design matrix A (one row per used sample) and the two right-hand sides
  penalty(grid, lam)               the second-difference penalty matrices, summed
  fit(...)                         measurements -> A -> (A^T A + penalties + mu I) c = A^T m + mu c_prior, a direct sparse solve, stats
  replay(ms, grid, w_max)          the kernel's fixed-point rule: every product rounded to 2^-32 and summed as an integer ->
                                   H [ncp][49 | 343] and b [2][ncp] as the kernel converts them back: bit for bit its H_out, b_out
  stencil_of(H, grid)              a sparse / dense ncp x ncp matrix in the kernel's stencil layout (matrix_of: back again)
  pcg(M, rhs, x0, k)               iterate k of the header's Jacobi-preconditioned CG for one component, fp64 or long double
  edge_history, edge_grid, ...     the inputs of tests/test_gpu_wind_fit_edges.py (the last section of this file)

A grid is a Grid(nt, ny, nx, t0, ht, x0, hx, y0, hy): the geometry of a d2d_wind_field (n control points, first knot u0, spacing h:
the box is [u0, u0 + (n - 3) h])."""
import collections

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from d2d.wind import _weights

Grid = collections.namedtuple('Grid', 'nt ny nx t0 ht x0 hx y0 hy')
CHUNK = 64
SCALE = 2.0 ** 32


def grid_of(field):
    """The Grid of a SplineWindField (or anything with cp, x0, hx, ...)."""
    nt, _, ny, nx = field.cp.shape
    return Grid(nt, ny, nx, field.t0, field.ht, field.x0, field.hx, field.y0, field.hy)


def grid_over(x, y, t=None):
    """The Grid whose box is [x[0], x[-1]] x [y[0], y[-1]] (x [t[0], t[-1]]) for uniform knot arrays: len + 2 control points."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    if t is None:
        return Grid(1, len(y) + 2, len(x) + 2, 0.0, 1.0, x[0], x[1] - x[0], y[0], y[1] - y[0])
    t = np.asarray(t, float)
    return Grid(len(t) + 2, len(y) + 2, len(x) + 2, t[0], t[1] - t[0], x[0], x[1] - x[0], y[0], y[1] - y[0])


def sincos(a):
    """(cos, sin) of a: Cody-Waite reduction by pi/2 in three parts, the fdlibm kernel polynomials, every operation rounded once."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        k = np.rint(a * 6.36619772367581382433e-01)
        r = ((a - k * 1.57079632673412561417e+00) - k * 6.07710050630396597660e-11) - k * 2.02226624879595063154e-21
        z = r * r
        ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04
             + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))))
        pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05
             + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))))
        sr = r + (r * z) * ps
        cr = 1.0 - (0.5 * z - (z * z) * pc)
        n = np.where(np.isfinite(k), k, 0.0).astype(np.int64) & 3
    c = np.select([n == 0, n == 1, n == 2], [cr, -sr, -cr], sr)
    s = np.select([n == 0, n == 1, n == 2], [sr, cr, -sr], -cr)
    return c, s


def _axis(u, u0, h, n):
    """inside the box?, segment, the four weights (d2d.wind._weights: the expressions of wind_axis; inside the box it clamps nothing)."""
    with np.errstate(invalid='ignore'):
        s = (u - u0) / h
        inside = (s >= 0.0) & (s <= n - 3.0)
    seg, b = _weights(np.where(inside, u, u0), u0, h, n)
    return inside, seg, b


def measure(X, n_ac, dt_row, grid, rows=None, t_start=None, w_max=50.0):
    """The samples of X [n_rows][5][N]: dict of arrays over (i, d) = (n_rows - 1, N) -- valid (both rows valid), why (0 used, 1 not
    finite, 2 outside, 3 above w_max; -1 not a sample), m (2, ...), px, py, tm, seg (3, ...) = (it, iy, ix), bt, by, bx (4, ...)."""
    X = np.asarray(X, dtype=np.float64)
    n_rows, _, N = X.shape
    n_form = N // n_ac
    rows_f = np.full(n_form, n_rows) if rows is None else np.clip(np.asarray(rows), 0, n_rows)
    t0 = np.zeros(n_form) if t_start is None else np.broadcast_to(np.asarray(t_start, dtype=np.float64), (n_form,))
    rows_d, t0_d = np.repeat(rows_f, n_ac), np.repeat(t0, n_ac)
    i = np.arange(n_rows - 1)[:, None]
    valid = i + 1 < rows_d[None, :]
    A, B = X[:-1], X[1:]
    with np.errstate(invalid='ignore', over='ignore'):
        fin = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1)
        tm = t0_d[None, :] + (i.astype(np.float64) + 0.5) * dt_row
        if grid.nt > 1:
            fin &= np.isfinite(tm)
        px, py = 0.5 * (A[:, 0] + B[:, 0]), 0.5 * (A[:, 1] + B[:, 1])
        inx, ix, bx = _axis(px, grid.x0, grid.hx, grid.nx)
        iny, iy, by = _axis(py, grid.y0, grid.hy, grid.ny)
        inside = inx & iny
        it, bt = np.zeros_like(ix), np.zeros((4,) + ix.shape)
        bt[0] = 1.0
        if grid.nt > 1:
            int_, it, bt = _axis(tm, grid.t0, grid.ht, grid.nt)
            inside &= int_
        c0, s0 = sincos(A[:, 2]); c1, s1 = sincos(B[:, 2])
        mx = (B[:, 0] - A[:, 0]) / dt_row - 0.5 * (A[:, 4] * c0 + B[:, 4] * c1)
        my = (B[:, 1] - A[:, 1]) / dt_row - 0.5 * (A[:, 4] * s0 + B[:, 4] * s1)
        over = ~((np.abs(mx) <= w_max) & (np.abs(my) <= w_max))
    why = np.where(~fin, 1, np.where(~inside, 2, np.where(over, 3, 0)))
    why = np.where(valid, why, -1)
    return dict(valid=valid, why=why, m=np.stack([mx, my]), px=px, py=py, tm=tm, seg=np.stack([it, iy, ix]), bt=bt, by=by, bx=bx,
                counts=[int((why == k).sum()) for k in range(4)])


def _rows_of(ms, grid):
    """Per used sample: the ncp indices (S, nw) and weights (S, nw) of its design row, nw = 16 or 64, in the kernel's order
    (c, a, b) with weight bt[c] (by[a] bx[b]) (steady: by[a] bx[b])."""
    use = ms['why'] == 0
    it, iy, ix = (s[use] for s in ms['seg'])
    bt, by, bx = (b[:, use] for b in (ms['bt'], ms['by'], ms['bx']))
    kt = 4 if grid.nt > 1 else 1
    idx, w = [], []
    for c in range(kt):
        for a in range(4):
            for b in range(4):
                idx.append(((it + c) * grid.ny + iy + a) * grid.nx + ix + b)
                w2 = by[a] * bx[b]
                w.append(bt[c] * w2 if kt == 4 else w2)
    return np.stack(idx, 1), np.stack(w, 1), ms['m'][:, use]


def design(ms, grid):
    """(A sparse (S, ncp), m (2, S))."""
    idx, w, m = _rows_of(ms, grid)
    S, nw = idx.shape
    ncp = grid.nt * grid.ny * grid.nx
    A = sp.csr_matrix((w.ravel(), (np.repeat(np.arange(S), nw), idx.ravel())), shape=(S, ncp))
    return A, m


def _d2(n):
    """second differences at the interior points of an axis of n control points: (n - 2, n)"""
    return sp.diags([np.ones(n - 2), -2.0 * np.ones(n - 2), np.ones(n - 2)], [0, 1, 2], shape=(n - 2, n))


def penalty(grid, lam):
    """lam_x Dx^T Dx + lam_y Dy^T Dy + lam_t Dt^T Dt over the control points ordered (t, y, x)."""
    lam = (lam,) * 3 if np.ndim(lam) == 0 else lam
    It, Iy, Ix = sp.identity(grid.nt), sp.identity(grid.ny), sp.identity(grid.nx)
    Dx = sp.kron(It, sp.kron(Iy, _d2(grid.nx)))
    Dy = sp.kron(It, sp.kron(_d2(grid.ny), Ix))
    P = lam[0] * (Dx.T @ Dx) + lam[1] * (Dy.T @ Dy)
    if grid.nt > 1:
        Dt = sp.kron(_d2(grid.nt), sp.kron(Iy, Ix))
        P = P + lam[2] * (Dt.T @ Dt)
    return sp.csr_matrix(P)


def _prior_vec(grid, prior):
    ncp = grid.nt * grid.ny * grid.nx
    if prior is None:
        return np.zeros((2, ncp))
    pr = np.asarray(prior, dtype=np.float64)
    if pr.shape == (2,):
        return np.repeat(pr[:, None], ncp, 1)
    return pr.reshape(grid.nt, 2, grid.ny * grid.nx).transpose(1, 0, 2).reshape(2, ncp)


def system(H, b, grid, lam, mu, prior=None):
    """(M, rhs (2, ncp)) of the solve from H (ncp x ncp) and b (2, ncp)."""
    ncp = grid.nt * grid.ny * grid.nx
    M = sp.csc_matrix(sp.csr_matrix(H) + penalty(grid, lam) + mu * sp.identity(ncp))
    return M, b + mu * _prior_vec(grid, prior)


def fit(X, n_ac, dt_row, grid, rows=None, t_start=None, w_max=50.0, lam=1e-2, mu=1e-6, prior=None):
    """The estimator: dict(cp (nt, 2, ny, nx), c (2, ncp), support, stats (8; the two CG numbers 0), H (sparse), b, ms, A)."""
    ms = measure(X, n_ac, dt_row, grid, rows, t_start, w_max)
    A, m = design(ms, grid)
    H = (A.T @ A).tocsr()
    b = np.stack([A.T @ m[0], A.T @ m[1]])
    M, rhs = system(H, b, grid, lam, mu, prior)
    lu = spl.splu(M)
    c = np.stack([lu.solve(rhs[0]), lu.solve(rhs[1])])
    res = np.stack([A @ c[0] - m[0], A @ c[1] - m[1]])
    stats = np.array(ms['counts'] + [float(res[0] @ res[0]), float(res[1] @ res[1]), 0.0, 0.0], dtype=np.float64)
    cp = c.reshape(2, grid.nt, grid.ny, grid.nx).transpose(1, 0, 2, 3).copy()
    return dict(cp=cp, c=c, support=np.asarray(H.diagonal()), stats=stats, H=H, b=b, ms=ms, A=A)


def w_pow2(w_max):
    """w_max rounded up to a power of two: the scale of the right-hand side's fixed point."""
    fr, e = np.frexp(w_max)
    return float(np.ldexp(1.0, e - 1 if fr == 0.5 else e))


def stencil_index(grid):
    """For every (p, st): the partner's control-point index, -1 outside the grid: (ncp, 49 | 343)."""
    kt = 4 if grid.nt > 1 else 1
    it, iy, ix = np.meshgrid(np.arange(grid.nt), np.arange(grid.ny), np.arange(grid.nx), indexing='ij')
    offs = [(dt, dy, dx) for dt in (range(-3, 4) if kt == 4 else (0,)) for dy in range(-3, 4) for dx in range(-3, 4)]
    out = np.full((grid.nt * grid.ny * grid.nx, len(offs)), -1, dtype=np.int64)
    for st, (dt, dy, dx) in enumerate(offs):
        qt, qy, qx = it + dt, iy + dy, ix + dx
        ok = (qt >= 0) & (qt < grid.nt) & (qy >= 0) & (qy < grid.ny) & (qx >= 0) & (qx < grid.nx)
        out[:, st] = np.where(ok, (qt * grid.ny + qy) * grid.nx + qx, -1).ravel()
    return out


def stencil_of(H, grid):
    """A ncp x ncp matrix (sparse or dense) in the kernel's layout [ncp][49 | 343] (0 where the partner is outside the grid)."""
    Hd = np.asarray(H.todense()) if sp.issparse(H) else np.asarray(H)
    q = stencil_index(grid)
    p = np.arange(q.shape[0])[:, None]
    return np.where(q >= 0, Hd[p, np.maximum(q, 0)], 0.0)


def replay(ms, grid, w_max):
    """The kernel's sums: every w_i w_j rounded to a multiple of 2^-32 (np.rint of w_i (2^32 w_j): to nearest even, as the kernel's
    rint), every w_i (m / W) likewise, int64 sums, converted back as the kernel does.  Returns H (ncp, 49 | 343), b (2, ncp),
    and the integer sums Hq, bq."""
    idx, w, m = _rows_of(ms, grid)
    S, nw = idx.shape
    ncp = grid.nt * grid.ny * grid.nx
    W = w_pow2(w_max)
    Hq = np.zeros((ncp, ncp), dtype=np.int64)
    bq = np.zeros((2, ncp), dtype=np.int64)
    if S:
        prod = np.rint(w[:, :, None] * (w[:, None, :] * SCALE)).astype(np.int64)         # row i: w_i, column j: the lane's own w_j 2^32
        np.add.at(Hq, (idx[:, :, None].repeat(nw, 2), idx[:, None, :].repeat(nw, 1)), prod)
        for k in range(2):
            np.add.at(bq[k], idx, np.rint((w * SCALE) * (m[k] * (1.0 / W))[:, None]).astype(np.int64))
    q = stencil_index(grid)
    p = np.arange(ncp)[:, None]
    Hs = np.where(q >= 0, Hq[p, np.maximum(q, 0)], 0)
    return Hs.astype(np.float64) * (1.0 / SCALE), bq.astype(np.float64) * (1.0 / SCALE) * W, Hs, bq


def field_at(cp, grid, t, x, y):
    """The spline with control points cp (nt, 2, ny, nx) at arrays t, x, y -> (wx, wy)."""
    from d2d.wind import SplineWindField
    return SplineWindField(cp, grid.x0, grid.hx, grid.y0, grid.hy, grid.t0, grid.ht).sample_many(t, x, y)


# ---- the recovery cases shared by tests/test_wind_fit_cpu.py (which measures them) and tests/test_gpu_wind_fit.py ------------------
RECOVERY_STEPS, RECOVERY_DT = 120, 0.05
RECOVERY_C = np.array([[0, -20], [25, -40], [25, -80], [0, -100.0]])
RECOVERY_R, RECOVERY_V = 60.0, 15.0
RECOVERY_ERR = {'shear': 6.5e-3, 'gust': 3.3e-2}     # m/s: measured by tests/test_wind_fit_cpu.py test_recovery_of_truth (6.41e-3, 3.23e-2)


def recovery_x0():
    X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (4, 1))
    X0[:, 0] += np.arange(4) * 7.0
    return X0


def recovery_case(name):
    """(truth F, Grid, knot arrays (x, y, t), lam) of the two recovery cases: 'shear' (tests/wind_ref.shear, steady) and 'gust'
    (wind_ref.gust, unsteady).  The grids cover the region the formation of RECOVERY_C flies in RECOVERY_STEPS rows."""
    import wind_ref as R
    x, y = np.arange(-80.0, 121.0, 40.0), np.arange(-160.0, 81.0, 40.0)
    if name == 'shear':
        return R.spline_of(R.shear), grid_over(x, y), (x, y, None), 1e-2
    t = np.arange(0.0, 8.1, 2.0)
    return R.spline_of(R.gust, t=np.arange(0.0, 21.0, 2.0)), grid_over(x, y, t), (x, y, t), 1e-3


def recovery_error(cp, grid, F, ms):
    """The largest |F^ - F| over the used samples' midpoints and times, and the largest |m - F| there (the measurement's own error)."""
    use = ms['why'] == 0
    fx, fy = field_at(cp, grid, ms['tm'][use], ms['px'][use], ms['py'][use])
    tx, ty = F.sample_many(ms['tm'][use], ms['px'][use], ms['py'][use])
    return (max(np.abs(fx - tx).max(), np.abs(fy - ty).max()),
            max(np.abs(ms['m'][0][use] - tx).max(), np.abs(ms['m'][1][use] - ty).max()))


# ---- the geometry-edge cases shared by tests/test_wind_fit_cpu.py (which proves what each input is) and
# ---- tests/test_gpu_wind_fit_edges.py (which holds the kernels to replay() on them) -------------------------------------------------
EDGE_ROWS, EDGE_DT, EDGE_W_MAX = 130, 0.05, 30.0
EDGE_LAM, EDGE_MU, EDGE_CG_TOL, EDGE_CG_MAX = (1e-2, 2e-2, 5e-3), 1e-4, 1e-10, 4000
EDGE_SHAPES = {                                        # (n_form, n_ac) -> (rows, t_start)
    (3, 3): ([130, 65, 2], [0.0, 3.0, 7.5]),           # N = 9: the last quad holds one drone, quads straddle formations
    (2, 5): ([66, 64], [0.0, 7.5]),                    # N = 10: the last quad holds two; one unit plus two samples, one unit exactly
    (1, 1): ([129], [2.0]),                            # three of a workgroup's four wavefronts leave at once
    (1, 64): ([129], [2.0]),                           # the largest formation
}
EDGE_BIG = dict(shape=(3, 4), rows=[40, 30, 33], t_start=[0.0, 3.0, 12.0], corners=(3, 11))     # about 400 samples for the large grids
EDGE_BIG_GRIDS = {'steady-23x29': (1, 23, 29), 'unsteady-5x11x13': (5, 11, 13), 'steady-64x64': (1, 64, 64), 'unsteady-4x32x32': (4, 32, 32)}


def edge_grid(nt, ny, nx):
    """The Grid of nt x ny x nx control points whose box is x in [-120, 120], y in [-100, 100] (t in [-1, 15]): around edge_history."""
    return Grid(nt, ny, nx, -1.0 if nt > 1 else 0.0, 16.0 / (nt - 3) if nt > 1 else 1.0, -120.0, 240.0 / (nx - 3), -100.0, 200.0 / (ny - 3))


def edge_history(n_form, n_ac, seed=5, corners=None):
    """[EDGE_ROWS][5][n_form n_ac]: drones on arcs through a wind that varies in space (not a simulation: any history is one).  The
    recorded headings carry offsets of both signs up to 1e5 (the positions are integrated from the recorded heading, so the
    measurements stay the wind).  With three drones or more: drone 0 has a NaN row, drone 1 leaves the box, drone 2 jumps (a
    measurement above w_max).  corners = (d_lo, d_hi): those two start half a metre inside the box's lower and upper corner and fly
    inwards, so that the first and the last cell of every grid of edge_grid hold samples."""
    rng = np.random.default_rng(seed)
    N = n_form * n_ac
    t = np.arange(EDGE_ROWS) * EDGE_DT
    X = np.zeros((EDGE_ROWS, 5, N))
    offs = (0.0, -40.0 * np.pi, 1e5, -1e5 - 3.0, 80.0 * np.pi)
    for d in range(N):
        v, om, psi0, xs, ys = rng.uniform(9.0, 14.0), rng.uniform(-0.35, 0.35), rng.uniform(-np.pi, np.pi), rng.uniform(-25.0, 25.0), rng.uniform(-20.0, 20.0)
        off = offs[d % 5]
        if N >= 3 and d == 1:
            om, psi0, xs, off = 0.0, 0.0, 110.0, 0.0                  # straight out of the box through x = 120
        if corners is not None and d == corners[0]:
            v, om, psi0, xs, ys = 10.0, 0.0, 0.25 * np.pi, -119.5, -99.5
        if corners is not None and d == corners[1]:
            v, om, psi0, xs, ys = 10.0, 0.0, -0.75 * np.pi, 119.5, 99.5
        psi = (psi0 + om * t) + off
        x = xs + np.cumsum(np.r_[0.0, (v * np.cos(psi[:-1]) + 2.0) * EDGE_DT])
        y = ys + np.cumsum(np.r_[0.0, (v * np.sin(psi[:-1]) - 1.0 + 0.02 * x[:-1]) * EDGE_DT])
        X[:, 0, d], X[:, 1, d], X[:, 2, d], X[:, 3, d], X[:, 4, d] = x, y, psi, 0.1 * om, v
    if N >= 3:
        X[17, 3, 0] = np.nan
        X[70:, 1, 2] += 4.0
    return X


def edge_prior(grid, y_shift=0.0):
    """A prior [nt][2][ny][nx] that differs in every entry: a transposed or mis-strided plane shows.  y_shift moves the y planes only."""
    t, k, y, x = np.meshgrid(np.arange(grid.nt), np.arange(2), np.arange(grid.ny), np.arange(grid.nx), indexing='ij')
    return 1.0 + 0.1 * t + 10.0 * k + 0.7 * y + 0.09 * x + y_shift * k


def zero_rhs_history(n_ac=4, n_rows=40):
    """Due east (psi = 0 exactly) at constant y: sin(0) = 0 in sincos, so every m_y is exactly 0 and the y right-hand side is too."""
    X = np.zeros((n_rows, 5, n_ac))
    t = np.arange(n_rows) * EDGE_DT
    for d in range(n_ac):
        X[:, 0, d] = -60.0 + 7.0 * d + (11.0 + d + 2.0) * t
        X[:, 1, d] = -30.0 + 25.0 * d
        X[:, 4, d] = 11.0 + d
    return X


SAMPLE_EDGE_DT = 0.0625
SAMPLE_EDGE_ROWS = [3, 2, 3, 3]                        # four formations of one drone, three rows
SAMPLE_EDGE_COUNTS = {32.0: [5, 0, 1, 1], 33.0: [6, 0, 1, 0], 30.0: [4, 0, 1, 2]}       # w_max -> used, not finite, outside, over: by hand


def sample_edge_case(origin=False):
    """(X [3][5][4], Grid) of the hand-built history on the 5 x 6 grid, dt_row = 1 / 16; every number is exact in binary.
      drone 0  v = 0; the first midpoint is the box's upper corner exactly (used, segment n - 4, r = 1: 16 m/s), the second is outside
      drone 1  v = 0; two rows: the midpoint is the box's lower corner exactly
      drone 2  v = 0, 2 m a row: m_x = 32 exactly (used at w_max >= 32), then 2 + 2^-40 m: m_x = 32 + 2^-36 (over at w_max = 32)
      drone 3  psi = -1e6, 1e6, -0.0 at 10 m/s
    origin: the box's lower corner moved to (0, 0) (every coordinate shifted exactly) and drone 1 parked at (-0.0, -0.0): the lower
    edge reached through s = -0.0."""
    g = Grid(1, 5, 6, 0.0, 1.0, -120.0, 80.0, -100.0, 100.0)
    X = np.zeros((3, 5, 4))
    X[:, 0, 0], X[:, 1, 0], X[:, 2, 0] = [119.5, 120.5, 121.5], [99.5, 100.5, 101.5], 0.3
    X[:, 0, 1], X[:, 1, 1] = [-120.5, -119.5, 0.0], [-100.5, -99.5, 0.0]
    X[:, 0, 2], X[:, 1, 2] = [0.0, 2.0, 4.0 + 2.0 ** -40], 10.0
    X[:, 0, 3], X[:, 1, 3], X[:, 2, 3], X[:, 4, 3] = [-50.0, -49.75, -49.5], [-50.0, -50.125, -50.25], [-1e6, 1e6, -0.0], 10.0
    if origin:
        X[:, 0] += 120.0; X[:, 1] += 100.0
        X[:, 0, 1] = X[:, 1, 1] = -0.0
        g = g._replace(x0=0.0, y0=0.0)
    return X, g


def matrix_of(Hs, grid):
    """The inverse of stencil_of: the sparse ncp x ncp matrix of a stencil array [ncp][49 | 343]."""
    q = stencil_index(grid)
    on = q >= 0
    p = np.broadcast_to(np.arange(q.shape[0])[:, None], q.shape)
    return sp.csr_matrix((np.asarray(Hs)[on], (p[on], q[on])), shape=(q.shape[0],) * 2)


def replay_blocks(ms, grid, w_max, block=8):
    """replay for a history of many drones: `block` drones at a time, the integer sums added (they are integers: exactly what the
    kernel's atomics do), so that the S x 64 x 64 product array stays small.  Returns H, b as replay does."""
    N = ms['why'].shape[1]
    Hq = bq = None
    for d0 in range(0, N, block):
        why = np.full_like(ms['why'], -1)
        why[:, d0:d0 + block] = ms['why'][:, d0:d0 + block]
        _, _, hq, q = replay(dict(ms, why=why), grid, w_max)
        Hq, bq = (hq, q) if Hq is None else (Hq + hq, bq + q)
    return Hq.astype(np.float64) * (1.0 / SCALE), bq.astype(np.float64) * (1.0 / SCALE) * w_pow2(w_max)


def pcg(M, rhs, x0, k, tol=0.0, longdouble=False):
    """Iterate k of the solve as include/d2d.h states it, for ONE component: Jacobi-preconditioned conjugate gradients from x0, frozen
    once |r| <= tol |rhs| (a zero right-hand side with x0 = 0 is frozen at once) or when p^T M p is not positive.  Plain numpy, in
    fp64 or (longdouble) in np.longdouble with the same M, rhs and x0."""
    ty = np.longdouble if longdouble else np.float64
    Md = np.asarray(M.todense() if sp.issparse(M) else M).astype(ty)
    b, x = np.asarray(rhs).astype(ty), np.asarray(x0).astype(ty).copy()
    dinv = 1.0 / np.diag(Md)
    r = b - Md @ x
    p = dinv * r
    rz, bb = r @ p, b @ b
    for _ in range(k):
        if r @ r <= ty(tol) * ty(tol) * bb:
            break
        Ap = Md @ p
        pa = p @ Ap
        if not pa > 0.0:
            break
        al = rz / pa
        x, r = x + al * p, r - al * Ap
        z = dinv * r
        nz = r @ z
        p, rz = z + (nz / rz) * p, nz
    return x
