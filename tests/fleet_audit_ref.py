"""CPU statement of d2d_fleet_audit (include/d2d.h), plain numpy loops: brute force over every pair of aircraft of different formations.

A history X [n_rows][5][N] (drone d = formation d // n_ac), rows[f] valid rows, row i of formation f at the global row row0[f] + i;
formation f is valid at the global row g when 0 <= g - row0[f] < rows[f].  For aircraft A and B of different formations of the same
world, with p = B - A: at every g at which both are valid the row's own |p0|^2 is a candidate at time g, and if both are valid at
g + 1 so is the interior closest approach (flight_audit_ref.closest) at g + s*.  A candidate counts when its squared distance is
below d_look^2, strictly; the answer is the smallest key (d^2, g + s, B's global index), the root drawn at the end, the time
(g + s) dt_row.  A refused formation (status bits below) is absent for everybody else.
"""
import numpy as np

from flight_audit_ref import closest

NONFINITE, STEP, BAD_ROW0, RANGE = 1, 2, 4, 8
EDGE_MARGIN = 2.0 ** -16          # the relative inflation of the grid's cell edge, which the RANGE rule is stated with
CELL_MAX = 2.0 ** 30


def statuses(X, n_ac, d_look, step_max, rows_a, row0_a, g_rows, mg=None):
    """The refusal bits of every formation, each condition on its own."""
    n_rows, _, N = X.shape
    n_form = N // n_ac
    inv_edge = 1.0 / ((d_look + 2.0 * step_max) * (1.0 + EDGE_MARGIN)) if np.isfinite(d_look) else 0.0
    st = np.zeros(n_form, np.int32)
    with np.errstate(invalid='ignore', over='ignore'):
        for f in range(n_form):
            R = int(rows_a[f])
            P = X[:R, :2, f * n_ac:(f + 1) * n_ac]
            if not np.isfinite(P).all():
                st[f] |= NONFINITE
            if (np.abs(P * inv_edge) > CELL_MAX).any():
                st[f] |= RANGE
            if R > 1:
                dP = np.diff(P, axis=0)
                s2 = dP[:, 0] * dP[:, 0] + dP[:, 1] * dP[:, 1]
                if (s2 > step_max * step_max).any():
                    st[f] |= STEP
                if mg is not None and np.isfinite(s2).all():
                    mg['step'] = min(mg['step'], np.abs(np.sqrt(s2) - step_max).min())
            if row0_a[f] < 0 or int(row0_a[f]) + R > g_rows:
                st[f] |= BAD_ROW0
    return st


def audit(X, n_ac, dt_row, d_look, step_max, rows=None, row0=None, world=None, d_safe=0.0, g_rows=None, margins=None):
    """Returns the dictionary of Context.fleet_audit as numpy arrays.  d_look may be +inf here (the device call wants it finite).
    margins: a dict that receives how close the inputs come to a decision that rounding could turn -- 'look': the smallest
    | distance - d_look | of any candidate, 'count': the smallest | nearest distance at a row - d_safe |, 'partner': the smallest gap
    between an aircraft's nearest and second-nearest partner's closest approach (partners within d_look), 'step': the smallest
    | step - step_max |."""
    mg = dict(look=np.inf, count=np.inf, partner=np.inf, step=np.inf)
    X = np.asarray(X, dtype=np.float64)
    n_rows, _, N = X.shape
    n_form = N // n_ac
    rows_a = np.full(n_form, n_rows) if rows is None else np.clip(np.asarray(rows), 0, n_rows)
    row0_a = np.zeros(n_form, np.int64) if row0 is None else np.asarray(row0, dtype=np.int64)
    world_a = np.zeros(n_form, np.int64) if world is None else np.asarray(world, dtype=np.int64)
    if g_rows is None:
        g_rows = n_rows if row0 is None else max(int((row0_a + rows_a).max()), 1)
    st = statuses(X, n_ac, d_look, step_max, rows_a, row0_a, g_rows, mg)
    out = dict(near_dist=np.full(N, np.inf), near_partner=np.full(N, -1, np.int32), near_time=np.full(N, np.nan),
               near_count=np.zeros(N, np.int32), status=st)
    look2 = d_look * d_look
    for f in range(n_form):
        sl = slice(f * n_ac, (f + 1) * n_ac)
        if st[f]:
            out['near_dist'][sl] = out['near_time'][sl] = np.nan
            out['near_partner'][sl] = out['near_count'][sl] = -1
            continue
        for d in range(f * n_ac, (f + 1) * n_ac):
            best = None
            near = np.full(g_rows, np.inf)                       # the nearest other-formation aircraft AT each global row, squared
            per = []
            for e in range(N):
                fe = e // n_ac
                if fe == f or st[fe] or world_a[fe] != world_a[f]:
                    continue
                pair = None
                for g in range(g_rows):
                    i, ie = g - row0_a[f], g - row0_a[fe]
                    if not (0 <= i < rows_a[f] and 0 <= ie < rows_a[fe]):
                        continue
                    p0 = X[ie, :2, e] - X[i, :2, d]
                    r2 = p0[0] * p0[0] + p0[1] * p0[1]
                    near[g] = min(near[g], r2)
                    cands = [(r2, float(g), e)]
                    if i + 1 < rows_a[f] and ie + 1 < rows_a[fe]:
                        c = closest(p0, X[ie + 1, :2, e] - X[i + 1, :2, d])
                        if c is not None:
                            cands.append((c[1], g + c[0], e))
                    for k in cands:
                        mg['look'] = min(mg['look'], abs(np.sqrt(k[0]) - d_look))
                        if k[0] < look2:
                            pair = k if pair is None else min(pair, k)
                if pair is not None:
                    per.append(np.sqrt(pair[0]))
                    best = pair if best is None else min(best, pair)
            if len(per) > 1:
                per.sort()
                mg['partner'] = min(mg['partner'], per[1] - per[0])
            if best is not None:
                out['near_dist'][d], out['near_time'][d], out['near_partner'][d] = np.sqrt(best[0]), best[1] * dt_row, best[2]
            if d_safe > 0:
                out['near_count'][d] = int((near < d_safe * d_safe).sum())
                mg['count'] = min(mg['count'], np.abs(np.sqrt(near) - d_safe).min(initial=np.inf))
    if margins is not None:
        margins.update(mg)
    return out


def pair_distance(X, dt_row, d, e, t, row0_d=0, row0_e=0):
    """The distance between drones d and e at time t = (g + s) dt_row (both linear between their rows)."""
    u = t / dt_row
    g = int(np.floor(u + 1e-12))
    s = u - g
    i, ie = g - row0_d, g - row0_e
    p0 = X[ie, :2, e] - X[i, :2, d]
    if s <= 1e-12:
        return float(np.hypot(*p0))
    p1 = X[ie + 1, :2, e] - X[i + 1, :2, d]
    return float(np.hypot(*(p0 + s * (p1 - p0))))
