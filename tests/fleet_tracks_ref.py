"""CPU statement of d2d_fleet_tracks (include/d2d.h), plain numpy loops: brute force over every pair of aircraft of different formations.

History, clocks, worlds and refusals are those of fleet_audit_ref (whose status rule and segment rule are imported, not copied).
Formations are ranked by (prio[f], f), smaller first.  For formation f, C(f) holds every aircraft B of another, non-refused formation
of f's world with a smaller (prio, formation) for which some aircraft A of f and some candidate -- the row's own |p0|^2 at time g, or
the interior closest approach (fleet_audit_ref.closest) at g + s* -- has d^2 < d_look^2, strictly.  B's key is the smallest
(d^2, g + s, A); C(f) is ordered by (key, B) and its first n_mov members are written:

  knot k of f     at the global row g_k = row0[f] + (k (rows[f] - 1)) // (n_knot - 1), time t0 + g_k * dt_row (a product, then a sum),
                  position: B's history at its local row clip(g_k - row0[fB], 0, rows[fB] - 1)
  chord_err       over the global rows g of f's window at which B has a row: with k the largest index <= n_knot - 2 with g_k <= g,
                  s = (g - g_k) / (g_k+1 - g_k); px = xa + s * (xb - xa); py likewise; e2 = (x - px) * (x - px) + (y - py) * (y - py) --
                  every operation a rounded double operation of its own, in this order; chord_err = sqrt(max e2)
  absent slots    partner -1, part_dist +inf, part_time NaN, chord_err 0, disc (0, kind), the knot times above with positions 0
  status != 0     (the FLEET bits, or SHORT = 16: rows[f] < n_knot) n_conf -1, partners -1, NaN, discs absent, knot k at row0[f] + k.
                  A formation with a FLEET bit is absent for everybody else; one that is only SHORT is seen.
"""
import numpy as np

import fleet_audit_ref as FL
from fleet_audit_ref import closest           # the segment rule: the audit's, imported

SHORT = 16


def knot_rows(r0, rows_f, n_knot):
    """The global rows of the knots of a formation whose window is rows_f >= 2 rows from r0."""
    return [int(r0) + (k * (int(rows_f) - 1)) // (n_knot - 1) for k in range(n_knot)]


def pair_key(X, d, e, i_lo, i_hi, off_d, off_e, seg_d, seg_e, look2, reach2):
    """The smallest (d2, u) of aircraft d against e over the global rows i_lo .. i_hi - 1 at which both are valid, or None.
    off_*: the formation's row0; seg_*: its row0 + rows (the first global row it no longer has).  reach2 = (d_look + 2 step_max)^2: a
    segment that starts farther apart has no candidate below d_look (include/d2d.h, the step bound), so closest is not called."""
    best = None
    for g in range(i_lo, i_hi):
        p0 = X[g - off_e, :2, e] - X[g - off_d, :2, d]
        r2 = p0[0] * p0[0] + p0[1] * p0[1]
        if not r2 < reach2:
            continue
        cands = [(r2, float(g))]
        if g + 1 < seg_d and g + 1 < seg_e:
            c = closest(p0, X[g + 1 - off_e, :2, e] - X[g + 1 - off_d, :2, d])
            if c is not None:
                cands.append((c[1], g + c[0]))
        for k in cands:
            if k[0] < look2 and (best is None or k < best):
                best = k
    return best


def chord_err(X, e, r0e, rows_e, r0f, rows_f, n_knot):
    """The stated operation sequence, on numpy float64 scalars."""
    gk = knot_rows(r0f, rows_f, n_knot)
    loc = lambda g: min(max(g - r0e, 0), rows_e - 1)           # noqa: E731
    worst = np.float64(0.0)
    for g in range(r0f, r0f + rows_f):
        if not 0 <= g - r0e < rows_e:
            continue
        k = 0
        while k < n_knot - 2 and gk[k + 1] <= g:
            k += 1
        xa, ya = X[loc(gk[k]), 0, e], X[loc(gk[k]), 1, e]
        xb, yb = X[loc(gk[k + 1]), 0, e], X[loc(gk[k + 1]), 1, e]
        s = np.float64(g - gk[k]) / np.float64(gk[k + 1] - gk[k])
        px = xa + s * (xb - xa)
        py = ya + s * (yb - ya)
        ex, ey = X[g - r0e, 0, e] - px, X[g - r0e, 1, e] - py
        worst = max(worst, ex * ex + ey * ey)
    return np.sqrt(worst)


def tracks(X, n_ac, dt_row, d_look, step_max, r_disc, rows=None, row0=None, world=None, prio=None, n_mov=8, n_knot=32, kind=1, t0=0.0,
           g_rows=None, full=False):
    """Returns the dictionary of Context.fleet_tracks as numpy arrays.  full: also 'members', per formation the whole ordered C(f) as
    (d2, u, A, B) tuples."""
    X = np.asarray(X, dtype=np.float64)
    n_rows, _, N = X.shape
    n_form = N // n_ac
    rows_a = np.full(n_form, n_rows) if rows is None else np.clip(np.asarray(rows), 0, n_rows)
    row0_a = np.zeros(n_form, np.int64) if row0 is None else np.asarray(row0, dtype=np.int64)
    world_a = np.zeros(n_form, np.int64) if world is None else np.asarray(world, dtype=np.int64)
    prio_a = np.arange(n_form) if prio is None else np.asarray(prio, dtype=np.int64)
    if g_rows is None:
        g_rows = n_rows if row0 is None else max(int((row0_a + rows_a).max()), 1)
    fleet = FL.statuses(X, n_ac, d_look, step_max, rows_a, row0_a, g_rows)
    st = fleet | np.where(rows_a < n_knot, SHORT, 0).astype(np.int32)
    look2, reach2 = d_look * d_look, (d_look + 2.0 * step_max) ** 2
    out = dict(knots=np.zeros((n_form, n_mov, n_knot, 3)), disc=np.zeros((n_form, n_mov, 2)), partner=np.full((n_form, n_mov), -1, np.int32),
               part_dist=np.full((n_form, n_mov), np.inf), part_time=np.full((n_form, n_mov), np.nan), chord_err=np.zeros((n_form, n_mov)),
               n_conf=np.zeros(n_form, np.int32), status=st.astype(np.int32))
    out['disc'][:, :, 1] = kind
    members = []
    for f in range(n_form):
        r0f, rf = int(row0_a[f]), int(rows_a[f])
        if st[f]:
            out['n_conf'][f] = -1
            out['part_dist'][f] = out['chord_err'][f] = np.nan
            for k in range(n_knot):
                out['knots'][f, :, k, 0] = t0 + np.float64(r0f + k) * dt_row
            members.append(None)
            continue
        gk = knot_rows(r0f, rf, n_knot)
        for k in range(n_knot):
            out['knots'][f, :, k, 0] = t0 + np.float64(gk[k]) * dt_row
        C = []
        for e in range(N):
            fe = e // n_ac
            if fe == f or fleet[fe] or world_a[fe] != world_a[f] or not (prio_a[fe], fe) < (prio_a[f], f):
                continue
            r0e, re = int(row0_a[fe]), int(rows_a[fe])
            lo, hi = max(r0f, r0e), min(r0f + rf, r0e + re)
            key = None
            for d in range(f * n_ac, (f + 1) * n_ac):
                k = pair_key(X, d, e, lo, hi, r0f, r0e, r0f + rf, r0e + re, look2, reach2)
                if k is not None and (key is None or k + (d,) < key):
                    key = k + (d,)
            if key is not None:
                C.append(key + (e,))
        C.sort()
        members.append(C)
        out['n_conf'][f] = min(len(C), n_mov + 1)
        for m, (d2, u, _, e) in enumerate(C[:n_mov]):
            fe = e // n_ac
            r0e, re = int(row0_a[fe]), int(rows_a[fe])
            out['partner'][f, m], out['part_dist'][f, m], out['part_time'][f, m] = e, np.sqrt(d2), u * dt_row
            out['disc'][f, m, 0] = r_disc
            for k in range(n_knot):
                out['knots'][f, m, k, 1:] = X[min(max(gk[k] - r0e, 0), re - 1), :2, e]
            out['chord_err'][f, m] = chord_err(X, e, r0e, re, r0f, rf, n_knot)
    if full:
        out['members'] = members
    return out


def lattice_history(n_form, n_ac, n_rows, seed, span=24):
    """A history on which the device's fused operations and this file's unfused ones give the same bits: start positions on whole
    metres within +-span, every aircraft moving +-2 m per row and axis.  A relative step is then 0 or +-4 m per axis, |d|^2 is 16 or 32,
    s* = num / |d|^2 is a dyadic fraction and every product and sum of the segment rule is exact.  Ties in d^2 are common on it."""
    rng = np.random.default_rng(seed)
    N = n_form * n_ac
    X = np.zeros((n_rows, 5, N))
    X[0, :2] = rng.integers(-span, span + 1, (2, N))
    X[1:, :2] = X[0, :2] + np.cumsum(rng.choice([-2.0, 2.0], (n_rows - 1, 2, N)), axis=0)
    X[:, 4] = 12.0
    return X


# ---- the CPU statement of full_sim.deconflict_plans: the tracks above and the collocation statements of tests/nlp_moving_ref.py ----------
def deconflict(rows, Ws, n_ac, h, d_sep, margin, d_look, step_max, world=None, prio=None, row0=None, n_knot=32, n_mov=8, max_rounds=4,
               t0=0.0, kind=1, max_sweeps=12):
    """rows (R n_ac, SCEN_STRIDE), Ws: list of R n_ac plans (N, 5).  The loop of full_sim.deconflict_plans, formation by formation:
    per round the tracks of the current plans, discs of radius d_sep + margin + chord_err, and a re-solve from the current plan of
    every formation that has partners and was never solved against them, lists another set of partners, or lists an aircraft of a
    formation whose plan the round before replaced.  Returns the plans and dict(replanned: the formations of each round, costs: the
    costs of each round's solves per aircraft, status likewise, tracks: each round's tracks)."""
    import nlp_moving_ref as M
    from d2d.opty_utils import MovingObstacle
    Ws = [np.array(w, dtype=np.float64) for w in Ws]
    R, N = len(Ws) // n_ac, Ws[0].shape[0]
    r0 = np.zeros(R, int) if row0 is None else np.asarray(row0, dtype=int)
    last, changed = [None] * R, [False] * R
    info = dict(replanned=[], costs=[], status=[], tracks=[])
    for _ in range(max_rounds):
        X = np.stack(Ws, axis=2)                                  # (N, 5, R n_ac): the plans as a history with dt_row = h
        tr = tracks(X, n_ac, h, d_look, step_max, d_sep + margin, row0=row0, world=world, prio=prio, n_mov=n_mov, n_knot=n_knot,
                    kind=kind, t0=t0)
        info['tracks'].append(tr)
        need = []
        for f in range(R):
            ps = sorted(int(e) for e in tr['partner'][f])
            if tr['n_conf'][f] > 0 and (ps != last[f] or any(e >= 0 and changed[e // n_ac] for e in ps)):
                need.append(f)
        if not need:
            break
        now, costs, status = [False] * R, [], []
        for f in need:
            mv = [MovingObstacle(tr['knots'][f, m, :, 0], tr['knots'][f, m, :, 1:], tr['disc'][f, m, 0] + tr['chord_err'][f, m], kind=kind)
                  for m in range(n_mov) if tr['partner'][f, m] >= 0]
            sl = slice(f * n_ac, (f + 1) * n_ac)
            ts = t0 + r0[f] * h
            if n_ac == 1:
                W, i1 = M.solve(M.problem(rows[f], mv, ts, N=N, h=h), Ws[f])
                new, infos = [W], [i1]
            else:
                new, infos, _, _ = M.solve_groups(rows[sl], mv, Ws[sl], t_start=ts, max_sweeps=max_sweeps, N=N, h=h)
            ok = all(i['status'] == 1 for i in infos)
            if ok:
                Ws[sl] = [np.array(w) for w in new]
            now[f] = ok
            last[f] = sorted(int(e) for e in tr['partner'][f])
            costs.append([i['cost'] for i in infos]); status.append([i['status'] for i in infos])
        changed = now
        info['replanned'].append(need); info['costs'].append(costs); info['status'].append(status)
    return Ws, info
