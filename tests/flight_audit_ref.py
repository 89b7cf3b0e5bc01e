"""CPU statement of d2d_flight_audit (include/d2d.h), plain numpy, written as loops over formations, segments and partners.

A history X [n_rows][5][N] (planes x, y, psi, phi, v; drone d = formation d // n_ac, aircraft d % n_ac), row i of formation f at
t_start[f] + i dt_row, rows[f] valid rows.  Between two rows every position is linear in s; for a relative position p(s) = p0 + s d

    s* = clamp(-(p0 . d) / (d . d), 0, 1)   (0 when d . d = 0),   q = p0 + s* d,   distance |q|,   time t_start + (i + s*) dt_row.

At s* = 0 and s* = 1 q is the row's own p0 and p1 exactly, so the candidates of a history are its valid rows and, per segment with
0 < s* < 1, the interior point; minima are taken over the keys (|q|^2, i + s*, partner) in lexicographic order -- the smallest
distance, then the earliest time, then the smallest partner -- and the square root is drawn at the end.
"""
import numpy as np

NONFINITE, BAD_TSTART, BAD_TRACK = 1, 2, 4


def closest(p0, p1):
    """The interior closest approach of the segment p0 -> p1 to the origin: (s*, |q|^2) when 0 < s* < 1, else None."""
    d = p1 - p0
    dd = d[0] * d[0] + d[1] * d[1]
    num = -(p0[0] * d[0] + p0[1] * d[1])
    if not (num > 0.0 and num < dd):
        return None
    s = num / dd
    q = p0 + s * d
    return s, q[0] * q[0] + q[1] * q[1]


def mov_centres(knots, t_start, n_rows, dt_row):
    """d2d_mov_sample's expression: knots [n_mov][n_knot][3] of one formation -> centres [n_mov][2][n_rows] at t_start + i dt_row."""
    n_mov, n_knot = knots.shape[:2]
    out = np.zeros((n_mov, 2, n_rows))
    for m in range(n_mov):
        kn = knots[m]
        for i in range(n_rows):
            t = t_start + i * dt_row
            k = 0
            for q in range(1, n_knot - 1):
                if kn[q, 0] <= t:
                    k = q
            (ta, xa, ya), (tb, xb, yb) = kn[k], kn[k + 1]
            u = max((t - ta) / (tb - ta), 0.0)
            out[m, 0, i] = xb if u >= 1.0 else xa + u * (xb - xa)
            out[m, 1, i] = yb if u >= 1.0 else ya + u * (yb - ya)
    return out


def track_bad(knots, disc):
    """The rules of d2d_nlp_solve_moving for one formation's tracks."""
    if not np.isfinite(knots).all():
        return True
    if not (np.diff(knots[:, :, 0], axis=1) > 0).all():
        return True
    return not np.isin(disc[:, 1], (0.0, 1.0)).all()


def _path_min(P, rows, best, j):
    """Fold the candidates of the relative path P [rows][2] into best = (d2, u, j); returns the rows' own squared distances."""
    r2 = np.zeros(rows)
    for i in range(rows):
        r2[i] = P[i, 0] * P[i, 0] + P[i, 1] * P[i, 1]
        best = min(best, (r2[i], float(i), j))
        if i + 1 < rows:
            c = closest(P[i], P[i + 1])
            if c is not None:
                best = min(best, (c[1], i + c[0], j))
    return best, r2


NOTHING = (np.inf, np.inf, 1 << 30)     # no candidate seen (u = inf only orders the fold; reported as NaN)


def audit(X, n_ac, dt_row, rows=None, t_start=None, x_ref=None, y_ref=None, static=None, knots=None, disc=None, d_safe=0.0,
          err_tol=np.inf, centres=None, margins=None):
    """static [n_form][n_stat][3]; knots [n_form][n_mov][n_knot][3], disc [n_form][n_mov][2]; centres [n_form][n_mov][2][n_rows]: the
    moving centres to use in place of mov_centres (a test hands the library's own).  Returns the dictionary of Context.flight_audit
    as numpy arrays.  margins: a dict that receives how close the inputs come to a decision that rounding could turn -- 'count': the
    smallest |distance - threshold| of any counted comparison (d_safe, clearance 0, err_tol), 'partner': the smallest gap between an
    aircraft's nearest and second-nearest partner's closest approach."""
    mg = dict(count=np.inf, partner=np.inf)
    X = np.asarray(X, dtype=np.float64)
    n_rows, _, N = X.shape
    n_form = N // n_ac
    rows_a = np.full(n_form, n_rows) if rows is None else np.clip(np.asarray(rows), 0, n_rows)
    t0_a = np.zeros(n_form) if t_start is None else np.broadcast_to(np.asarray(t_start, dtype=np.float64), (n_form,))
    n_stat = 0 if static is None else static.shape[1]
    n_mov = 0 if knots is None else knots.shape[1]
    out = dict(sep_dist=np.full(N, np.inf), sep_partner=np.full(N, -1, np.int32), sep_time=np.full(N, np.nan), sep_count=np.zeros(N, np.int32),
               phi_max=np.full(N, -np.inf), v_min=np.full(N, np.inf), v_max=np.full(N, -np.inf), status=np.zeros(n_form, np.int32))
    if n_stat:
        out.update(stat_clear=np.full((n_stat, N), np.inf), stat_time=np.full((n_stat, N), np.nan), stat_count=np.zeros((n_stat, N), np.int32))
    if n_mov:
        out.update(mov_clear=np.full((n_mov, N), np.inf), mov_time=np.full((n_mov, N), np.nan), mov_count=np.zeros((n_mov, N), np.int32))
    if x_ref is not None:
        out.update(err_max=np.full(N, -np.inf), err_time=np.full(N, np.nan), err_count=np.zeros(N, np.int32))
    for f in range(n_form):
        R, t0 = int(rows_a[f]), float(t0_a[f])
        sl = slice(f * n_ac, (f + 1) * n_ac)
        when = lambda u: t0 + u * dt_row      # noqa: E731
        # ---- refusals
        st = 0
        if not np.isfinite(X[:R, [0, 1, 3, 4], sl]).all():
            st |= NONFINITE
        if x_ref is not None and not (np.isfinite(x_ref[:R, sl]).all() and np.isfinite(y_ref[:R, sl]).all()):
            st |= NONFINITE
        for k in range(n_stat):
            if not static[f, k, 2] <= 0 and not np.isfinite(static[f, k]).all():
                st |= NONFINITE
        for m in range(n_mov):
            if not disc[f, m, 0] <= 0 and not np.isfinite(disc[f, m, 0]):
                st |= NONFINITE
        if not np.isfinite(t0):
            st |= BAD_TSTART
        if n_mov and track_bad(knots[f], disc[f]):
            st |= BAD_TRACK
        out['status'][f] = st
        if st:
            for k, v in out.items():
                if k != 'status':
                    v[..., sl] = np.nan if v.dtype == np.float64 else -1
            continue
        ctr = None
        if n_mov:
            ctr = centres[f] if centres is not None else mov_centres(knots[f], t0, n_rows, dt_row)
        for a in range(n_ac):
            d = f * n_ac + a
            P = X[:R, :2, d]
            # ---- separation
            best, near, per = NOTHING, np.full(R, np.inf), []
            for j in range(n_ac):
                if j != a:
                    bj, r2 = _path_min(X[:R, :2, f * n_ac + j] - P, R, NOTHING, j)
                    best = min(best, bj)
                    per.append(np.sqrt(bj[0]))
                    near = np.minimum(near, r2)
            if len(per) > 1 and R > 0:
                per.sort()
                mg['partner'] = min(mg['partner'], per[1] - per[0])
            if d_safe > 0 and R > 0:
                mg['count'] = min(mg['count'], np.abs(np.sqrt(near) - d_safe).min())
            if best is not NOTHING:
                out['sep_dist'][d], out['sep_time'][d], out['sep_partner'][d] = np.sqrt(best[0]), when(best[1]), best[2]
            if d_safe > 0:
                out['sep_count'][d] = int((near < d_safe * d_safe).sum())
            # ---- clearance
            for k in range(n_stat):
                cx, cy, r = static[f, k]
                if r <= 0:
                    continue
                best, r2 = _path_min(P - np.array([cx, cy]), R, NOTHING, 0)
                if best is not NOTHING:
                    out['stat_clear'][k, d], out['stat_time'][k, d] = np.sqrt(best[0]) - r, when(best[1])
                out['stat_count'][k, d] = int((r2 < r * r).sum())
                mg['count'] = min(mg['count'], np.abs(np.sqrt(r2) - r).min(initial=np.inf))
            for m in range(n_mov):
                r = disc[f, m, 0]
                if r <= 0:
                    continue
                best, r2 = _path_min(P - ctr[m, :, :R].T, R, NOTHING, 0)
                if best is not NOTHING:
                    out['mov_clear'][m, d], out['mov_time'][m, d] = np.sqrt(best[0]) - r, when(best[1])
                out['mov_count'][m, d] = int((r2 < r * r).sum())
                mg['count'] = min(mg['count'], np.abs(np.sqrt(r2) - r).min(initial=np.inf))
            # ---- tracking error, envelope: row-wise
            if x_ref is not None and R > 0:
                ex, ey = P[:, 0] - x_ref[:R, d], P[:, 1] - y_ref[:R, d]
                e2 = ex * ex + ey * ey
                i = int(np.argmax(e2))                      # the first of equal maxima
                out['err_max'][d], out['err_time'][d] = np.sqrt(e2[i]), when(float(i))
                out['err_count'][d] = int((e2 > err_tol * err_tol).sum())
                if np.isfinite(err_tol):
                    mg['count'] = min(mg['count'], np.abs(np.sqrt(e2) - err_tol).min())
            if R > 0:
                out['phi_max'][d] = np.abs(X[:R, 3, d]).max()
                out['v_min'][d], out['v_max'][d] = X[:R, 4, d].min(), X[:R, 4, d].max()
    if margins is not None:
        margins.update(mg)
    return out


def synthetic_history(n_form, n_ac, n_rows, seed, span=40.0, step=3.0):
    """Random walks for the tests: positions start within +-span and move up to `step` metres per row and axis; psi, phi, v plausible."""
    rng = np.random.default_rng(seed)
    N = n_form * n_ac
    X = np.zeros((n_rows, 5, N))
    X[:, :2] = rng.uniform(-span, span, (1, 2, N)) + np.cumsum(rng.uniform(-step, step, (n_rows, 2, N)), axis=0)
    X[:, 2] = rng.uniform(-3, 3, (n_rows, N))
    X[:, 3] = rng.uniform(-0.6, 0.6, (n_rows, N))
    X[:, 4] = rng.uniform(9, 15, (n_rows, N))
    return X


def pair_distance(X, n_ac, dt_row, d, j, t, t_start=0.0, rows=None):
    """The distance between drone d and aircraft j of its formation at time t (linear between the first `rows` rows)."""
    return float(np.hypot(*_at((X[:, :2, (d // n_ac) * n_ac + j] - X[:, :2, d])[:rows], (t - t_start) / dt_row)))


def disc_clearance(X, dt_row, d, centre, r, t, t_start=0.0, rows=None):
    """Distance of drone d from a disc's centre minus r at time t; centre (2,) or its rows [2][n_rows] (linear between them)."""
    c = np.asarray(centre, dtype=np.float64)
    P = X[:, :2, d] - (c if c.ndim == 1 else c.T)
    return float(np.hypot(*_at(P[:rows], (t - t_start) / dt_row))) - r


def _at(P, u):
    i = min(max(int(np.floor(u)), 0), len(P) - 1)
    s = u - i
    return P[i] if s == 0 or i + 1 >= len(P) else P[i] + s * (P[i + 1] - P[i])


def rowwise_min(X, n_ac):
    """The row-wise separation a user can compute today: per drone the smallest distance to a partner AT the rows."""
    n_rows, _, N = X.shape
    P = X[:, :2, :].reshape(n_rows, 2, N // n_ac, n_ac)
    D = np.sqrt(((P[..., :, None] - P[..., None, :]) ** 2).sum(1))          # [rows][form][a][j]
    D[..., np.arange(n_ac), np.arange(n_ac)] = np.inf
    return D.min(axis=(0, 3)).reshape(N)
