"""CPU statement of the collocation solver with HARD keep-out discs that MOVE (include/d2d.h d2d_nlp_solve_keepout_moving,
d2d_nlp_solve_groups_keepout; test infrastructure only).

It is tests/nlp_keepout_ref.py with one change: disc m's centre at node i is the node's own, ctr[m, i] = c_m(t_start + i h), so

    g_im = (x_i - ctr[m, i, 0])^2 + (y_i - ctr[m, i, 1])^2 - R_m^2 > 0,        d = p_i - ctr[m, i].

The centres are data -- no derivative is added.  The family of inequalities is nlp_keepout_ref.Discs, which is written on per-node
centres in the first place: merit, stationarity, right-hand side, Newton block, dual step, the exact quadratic ratio test, the start
rule, the refusals and the dual clip are one code for both statements (the names below are nlp_keepout_ref's disc_* functions), and
the loop is oracle.nlp.solve_general.  This file supplies the centres of tracks at the node times and what goes round the solve.
The refusals: a non-finite R or centre, an end pose with g <= 0 AT ITS OWN NODE'S TIME (node 0 against ctr[:, 0], node N - 1 against
ctr[:, N - 1]), a free node with g <= 0 after the start rule.  With centres that do not depend on i, solve() is nlp_keepout_ref.solve
bit for bit; with no discs it is oracle.nlp.solve.

  solve_groups      the sweep loop of nlp_groups_pairs_ref around solve(): every aircraft of the scenario holds the scenario's discs in the
                    uncoupled sweep and in every turn; each turn is a full solve from the aircraft's current nodes (the start rule moves
                    nodes on a boundary back to 1.01 R, the duals restart at mub / g).  An aircraft whose guess is refused refuses
                    the scenario, before the first solve; an aircraft that a LATER turn cannot start is reported refused alone
                    (status 3, its nodes those of its previous solve), as the device does (include/d2d.h).
  deconflict_hard   fleet_tracks_ref.deconflict's loop with the discs hard and R = sqrt((d_sep + margin)^2 + step_max^2) + chord_err.

The relative-chord bound (chord_bound): two aircraft whose relative positions at two consecutive rows are d0, d1 with |d0|, |d1| >= R
and |d1 - d0| <= s are never closer than sqrt(R^2 - (s / 2)^2) in between, positions linear in time.  step_max bounds one aircraft's step,
so s <= 2 step_max and R^2 = d^2 + step_max^2 keeps the continuous distance >= d.
"""
import numpy as np

import nlp_keepout_ref as K
from nlp_keepout_ref import Plain, ratio_disc, ST_NONFINITE, PUSH, _box_push, constant_centres      # noqa: F401  (the static statement's pieces)
from nlp_keepout_ref import disc_g as g_values, disc_start as start, disc_refused as refused      # noqa: F401
from nlp_keepout_ref import disc_barrier_value as barrier_value, disc_barrier_terms as barrier_terms      # noqa: F401
from oracle import nlp

NV = nlp.NV


def centres(moving, t_start, N, h):
    """(n, N, 2) centres of the tracks (objects with .at) at the node times t_start + i h, and their radii (n,) (.r: the node radius)."""
    t = t_start + np.arange(N) * h
    ctr = np.stack([o.at(t) for o in moving]) if len(moving) else np.zeros((0, N, 2))
    return ctr, np.array([o.r for o in moving], dtype=np.float64)


def solve(prob, W0, ctr, R, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL, opt_tol=nlp.OPT_TOL):
    """nlp_keepout_ref.solve outside the discs of centres ctr (n, N, 2) and node radii R (n,) (R <= 0: absent).  Returns W and the info
    of nlp_keepout_ref.solve (zk (n, N): the discs' duals).  A refused problem: W0 itself, status 3, NaN cost and feas."""
    return K.solve_discs(prob, W0, np.asarray(ctr, float).reshape(-1, prob.pb.N, 2), np.asarray(R, float).reshape(-1), rho0=rho0,
                         inner_max=inner_max, outer_max=outer_max, feas_tol=feas_tol, opt_tol=opt_tol)


def problem_of(pb, field=None, t_start=0.0):
    """The problem object solve() asks for: the oracle Problem in its constant wind, or in `field` with node 0 at t_start."""
    import nlp_wind_ref as Rw
    return Plain(pb) if field is None else Rw.FieldProblem(pb, field, t_start)


def solve_moving(pb, W0, moving, t_start=0.0, field=None, **kw):
    """solve() of the oracle Problem pb outside the tracks `moving` (objects with .at and .r = the node radius), node i at t_start + i h."""
    ctr, R = centres(moving, t_start, pb.N, pb.h)
    return solve(problem_of(pb, field, t_start), W0, ctr, R, **kw)


def solve_groups(rows, moving, W0s, field=None, t_start=0.0, max_sweeps=12, tol=1e-7, N=None, h=None, **kw):
    """One scenario of len(rows) aircraft with the partner sets of the rows' SC_PMASK, every aircraft outside the scenario's hard moving
    discs.  Returns Ws, infos, sweeps, moved of nlp_groups_pairs_ref.solve_groups; a scenario with an aircraft that is refused before
    its first solve is refused whole: the guesses, status 3 and NaN for every aircraft, 0 sweeps."""
    import nlp_groups_pairs_ref as P
    N = len(W0s[0]) if N is None else N
    pbs = [nlp.problem_from_row(r, N, h) for r in rows]
    ctr, R = centres(moving, t_start, N, h)

    def inner(a, pb, W0):
        return solve(problem_of(pb, field, t_start), W0, ctr, R, **kw)
    for pb, W0 in zip(pbs, W0s):                     # the scenario's refusal: every aircraft's start, before the first solve
        fixed, hasL, hasU = nlp._barrier_sets(pb)
        W = np.asarray(W0, float).copy()
        W[:, :2] = _box_push(W[:, :2], pb.lo[:, :2], pb.hi[:, :2], hasL[:, :2], hasU[:, :2])
        ok = np.isfinite(R).all() and np.isfinite(ctr).all()
        if len(R) and (not ok or refused(pb, ctr, R, start(pb, W, ctr, R))):
            bad = dict(cost=np.nan, feas=np.nan, inner=0, status=ST_NONFINITE)
            return [np.asarray(w, float).copy() for w in W0s], [dict(bad) for _ in rows], 0, 0.0
    return P.solve_groups(pbs, W0s, inner, P.masks_of(rows), max_sweeps=max_sweeps, tol=tol)


def hard_radius(d_sep, margin, step_max):
    """The node radius of deconflict_hard before chord_err: sqrt(d^2 + step_max^2) -- two aircraft move at most 2 step_max relative to
    each other between two rows, and chord_bound(R, 2 step_max) = d."""
    return float(np.sqrt((d_sep + margin) ** 2 + step_max ** 2))


def chord_bound(R, s):
    """The smallest distance from the origin of a segment whose ends are at least R away and at most s apart."""
    return float(np.sqrt(max(R * R - 0.25 * s * s, 0.0)))


def deconflict_hard(rows, Ws, n_ac, h, d_sep, margin, d_look, step_max, world=None, prio=None, row0=None, n_knot=32, n_mov=8, max_rounds=4,
                    t0=0.0, max_sweeps=12):
    """fleet_tracks_ref.deconflict with the discs HARD: per round the tracks of the current plans with node radius
    hard_radius(d_sep, margin, step_max) + chord_err, and a re-solve (solve_moving / solve_groups) of the formations the soft loop would
    re-solve.  A formation whose re-solve is refused (status 3) or does not converge keeps its plan.  Returns the plans and
    dict(replanned, costs, status, tracks, refused, not_converged)."""
    import fleet_tracks_ref as T
    from d2d.opty_utils import MovingObstacle
    Ws = [np.array(w, dtype=np.float64) for w in Ws]
    R, N = len(Ws) // n_ac, Ws[0].shape[0]
    r0 = np.zeros(R, int) if row0 is None else np.asarray(row0, dtype=int)
    last, changed = [None] * R, [False] * R
    info = dict(replanned=[], costs=[], status=[], tracks=[], refused=set(), not_converged=set())
    for _ in range(max_rounds):
        X = np.stack(Ws, axis=2)
        tr = T.tracks(X, n_ac, h, d_look, step_max, hard_radius(d_sep, margin, step_max), row0=row0, world=world, prio=prio, n_mov=n_mov,
                      n_knot=n_knot, kind=1, t0=t0)
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
            mv = [MovingObstacle(tr['knots'][f, m, :, 0], tr['knots'][f, m, :, 1:], tr['disc'][f, m, 0] + tr['chord_err'][f, m], kind=1)
                  for m in range(n_mov) if tr['partner'][f, m] >= 0]
            sl = slice(f * n_ac, (f + 1) * n_ac)
            ts = t0 + r0[f] * h
            if n_ac == 1:
                W, i1 = solve_moving(nlp.problem_from_row(rows[f], N, h), Ws[f], mv, ts)
                new, infos = [W], [i1]
            else:
                new, infos, _, _ = solve_groups(rows[sl], mv, Ws[sl], t_start=ts, max_sweeps=max_sweeps, N=N, h=h)
            ok = all(i['status'] == 1 for i in infos)
            if ok:
                Ws[sl] = [np.array(w) for w in new]
                info['refused'].discard(f); info['not_converged'].discard(f)
            elif any(i['status'] == ST_NONFINITE for i in infos):
                info['refused'].add(f)
            else:
                info['not_converged'].add(f)
            now[f] = ok
            last[f] = sorted(int(e) for e in tr['partner'][f])
            costs.append([i['cost'] for i in infos]); status.append([i['status'] for i in infos])
        changed = now
        info['replanned'].append(need); info['costs'].append(costs); info['status'].append(status)
    info['refused'], info['not_converged'] = sorted(info['refused']), sorted(info['not_converged'])
    return Ws, info


# ---- the problems of tests/test_nlp_keepout_moving_cpu.py and tests/test_gpu_nlp_keepout_moving.py -----------------------------------
H0 = K.H0
MAX_MOV = 8
STEP_N = (3, 5, 17, 64, 65, 121)
STEP_TAGS = ('cross', 'overtake', 'shear', 'many')
STEP_FIELD = 'shear'
STEP_T_START = 1.5                             # the tracks' times are absolute: every case starts away from 0
# (disc radius as a share of the leg, seed) of a case, chosen on the CPU with the statement alone as nlp_keepout_ref.STEP_CASES was
# (nlp_steps_ref.check over every budget: determined within TOL_CAP, the same path from the perturbed starts, still stepping after the
# budgets of one outer iteration -- at 3 and 5 nodes the budget (8, 1) may end on the convergence test, as there): the largest radius of
# 9, 8, 7, 6, 5 % (3 and 5 nodes: 9, 7, 5, 3 %) and then the first seed of 0 .. 11.  (121, 'overtake') has none on that grid -- its
# tolerance after the budget (5, 3) or (5, 4) is 1.0e-8 .. 3e-8 there -- and is the first of 4, 3, 10, 12 % and seeds 0 .. 15.  Not listed: (0.09, 0).
STEP_CASES = {(3, 'cross'): (0.03, 6), (3, 'overtake'): (0.07, 3), (3, 'shear'): (0.09, 8), (3, 'many'): (0.09, 4),
              (5, 'cross'): (0.05, 7), (5, 'overtake'): (0.05, 1), (5, 'shear'): (0.09, 6), (5, 'many'): (0.09, 5),
              (17, 'cross'): (0.06, 0), (17, 'shear'): (0.07, 6), (17, 'many'): (0.07, 1),
              (64, 'cross'): (0.06, 2), (64, 'overtake'): (0.07, 8), (64, 'shear'): (0.07, 1), (64, 'many'): (0.06, 0),
              (65, 'cross'): (0.06, 5), (65, 'overtake'): (0.06, 4), (65, 'shear'): (0.07, 0), (65, 'many'): (0.06, 1),
              (121, 'cross'): (0.08, 0), (121, 'overtake'): (0.10, 13), (121, 'shear'): (0.08, 1), (121, 'many'): (0.09, 2)}


class Track:
    """A piecewise-linear track with the node radius r of the hard constraint (what solve_moving and centres read)."""

    def __init__(self, t, xy, r):
        from d2d.opty_utils import MovingObstacle
        self.trk = MovingObstacle(t, xy, 1.0, kind=1)
        self.t, self.xy, self.r = self.trk.t, self.trk.xy, float(r)

    def at(self, t):
        return self.trk.at(t)

    def padded(self, n_knot):
        return self.trk.padded(n_knot)


def line_track(c_mid, vel, t_mid, T, r):
    """A disc that is at c_mid at the time t_mid and moves with the constant velocity vel, knots a second before the plan's start and a
    second after its end (t_mid - T / 2 - 1, t_mid + T / 2 + 1)."""
    c_mid, vel = np.asarray(c_mid, float), np.asarray(vel, float)
    ta, tb = t_mid - 0.5 * T - 1.0, t_mid + 0.5 * T + 1.0
    return Track((ta, tb), (c_mid + vel * (ta - t_mid), c_mid + vel * (tb - t_mid)), r)


def tables(tracks_per_problem, n_knot=3):
    """knots (B, MAX_MOV, n_knot, 3) and disc (B, MAX_MOV, 2) = (R, 1): every problem's tracks, then absent slots (R = 0) that hold a
    valid track, as d2d_fleet_tracks writes them."""
    B = len(tracks_per_problem)
    knots = np.zeros((B, MAX_MOV, n_knot, 3)); disc = np.zeros((B, MAX_MOV, 2)); disc[:, :, 1] = 1.0
    knots[:, :, :, 0] = np.arange(n_knot, dtype=float)
    for b, trs in enumerate(tracks_per_problem):
        for m, o in enumerate(trs):
            knots[b, m] = o.padded(n_knot); disc[b, m, 0] = o.r
    return knots, disc


def step_tracks(tag, pb, L, Rf=0.09):
    """The tracks of a step case, node 0 at STEP_T_START.  'cross' and 'shear': the binding disc of nlp_keepout_ref.step_discs, which
    crosses the leg from right to left at 4 m/s and is 0.3 R to the left of the axis at mid-leg at mid-time.  'overtake': the same disc
    0.3 R to the left of the axis, which starts 1.5 R behind p0 and ends 1.5 R beyond p1: it overtakes the aircraft along the leg.
    'many': MAX_MOV slots -- the crossing disc in slot 3, slots 2 and 5 absent, the others far away and moving."""
    T = (pb.N - 1) * pb.h
    tm = STEP_T_START + 0.5 * T
    mid = 0.5 * (pb.p0[:2] + pb.p1[:2]); leg = pb.p1[:2] - pb.p0[:2]; ll = float(np.hypot(*leg))
    nrm = np.array([-leg[1], leg[0]]) / ll; ax = leg / ll
    R = max(Rf * L, Rf)
    cross = line_track(mid + 0.3 * R * nrm, 4.0 * nrm, tm, T, R)
    if tag in ('cross', 'shear'):
        return [cross]
    if tag == 'overtake':
        return [line_track(mid + 0.3 * R * nrm, (ll + 3.0 * R) / T * ax, tm, T, R)]
    far = [line_track(mid + (3.0 + k) * L * np.array([np.cos(1.1 * k), np.sin(1.1 * k)]), 3.0 * np.array([np.sin(0.7 * k), np.cos(0.7 * k)]), tm, T, 0.5 * R)
           for k in range(MAX_MOV)]
    far[3] = cross
    far[2].r = 0.0; far[5].r = 0.0
    return far


def steps_case(cid, prob, W0, tracks):
    import nlp_steps_ref as S
    N = prob.pb.N
    ctr, R = centres(tracks, STEP_T_START, N, prob.pb.h)
    nz = (len(R) * N + 4) // 5

    def run(W0s, inner_max, outer_max):
        W, info = solve(prob, W0s[0][:N], ctr, R, inner_max=inner_max, outer_max=outer_max)
        return K.ext(W, info)[None], dict(inner=(info['inner'],), status=(info['status'],), path=tuple(info['path']), raw=info)
    return S.Case(cid, np.concatenate([W0, np.zeros((nz, 5))])[None], run,
                  lambda W: (prob.cost(W), float(np.abs(prob.constraints(W)).max())))


_launches = {}


def steps_launch(N, cases=None):
    """d2d_nlp_solve_keepout_moving, the launches of N nodes: the constant-wind cases in one device call, 'shear' in a second one.
    -> dict tag -> (case, row, tracks padded to MAX_MOV slots, prob)."""
    import nlp_wind_ref as Rw
    cases = STEP_CASES if cases is None else cases
    key = (N, tuple(sorted((k, v) for k, v in cases.items() if k[0] == N)))
    if key not in _launches:
        out = {}
        for tag in STEP_TAGS:
            Rf, seed = cases.get((N, tag), (0.09, 0))
            pb, r, W0, L = K.leg_problem(N, 1000 + 100 * STEP_TAGS.index(tag) + seed)
            prob = Rw.FieldProblem(pb, Rw.fields()[STEP_FIELD], STEP_T_START) if tag == 'shear' else Plain(pb)
            trs = step_tracks(tag, pb, L, Rf)
            trs = trs + [Track((0.0, 1.0), ((0.0, 0.0), (0.0, 0.0)), 0.0) for _ in range(MAX_MOV - len(trs))]
            out[tag] = (steps_case(f'keepmov-{N}-{tag}', prob, W0, trs), r, trs, prob)
        _launches[key] = out
    return _launches[key]


FULL_N = K.FULL_N
FULL_T_START = 2.0
FULL_VC = 3.0                                   # m/s: the speed of the full solves' disc across the leg


def full_launch(N):
    """Full solves at N nodes: the leg, the row and the user's disc (c, r, margin) of nlp_keepout_ref.full_launch(N)[0], with the disc
    MOVING: (a) across the leg from right to left at FULL_VC, at c when the aircraft is at mid-leg; (b) along the leg at FULL_VC against
    the aircraft, at c at the same time.  The node radius is d2d.opty_utils.MovingKeepOut.lowered: the relative chord.
    -> list of (prob, row, W0, [track], MovingKeepOut)."""
    from d2d.opty_utils import MovingKeepOut
    prob, row, W0, _, (c, ru, margin) = K.full_launch(N)[0]
    pb = prob.pb
    T = (N - 1) * pb.h
    tm = FULL_T_START + 0.5 * T
    leg = pb.p1[:2] - pb.p0[:2]; ll = float(np.hypot(*leg)); nrm = np.array([-leg[1], leg[0]]) / ll; ax = leg / ll
    out = []
    for vel in (FULL_VC * nrm, -FULL_VC * ax):
        ta, tb = tm - 0.5 * T - 1.0, tm + 0.5 * T + 1.0
        ko = MovingKeepOut((ta, tb), (c + vel * (ta - tm), c + vel * (tb - tm)), ru, margin)
        out.append((prob, row, W0, [Track(ko.t, ko.xy, ko.lowered(pb.hi[1, 4], pb.h))], ko))
    return out


# ---- groups: a coupled pair whose aircraft 0 meets a crossing hard disc (tests/test_gpu_groups_keepout.py) ------------------------------
GROUP_N = (17, 41)
GROUP_T_START = 1.0
GROUP_SWEEPS = 24


def pair_scenario(N, gap=9.0):
    """Two aircraft side by side `gap` m apart (inside rcol = 10 m: CostCollision acts along the leg) on legs that 12 m/s covers in
    (N - 1) H0 seconds, aircraft 1 to the right of aircraft 0, masks of the pair (0, 1); a hard disc of node radius 6 % of the leg
    (at least 1.2 m) comes from the left at 3 m/s and is 0.9 R to the left of aircraft 0's leg when the aircraft is at mid-leg: aircraft 0
    gives way to the right, towards aircraft 1, which the collision term then moves.  Aircraft 1 stays outside the disc on its own.
    -> rows (2, SCEN_STRIDE), guesses, [track]."""
    import d2dhip as D
    import nlp_moving_ref as M
    L = 12.0 * H0 * (N - 1)
    rows = np.stack([M.row(1, p0=(0.0, 0.0, 0.0), p1=(L, 0.0, 0.0), N=N, kobs=0.0, obj_scale=0.5),
                     M.row(1, p0=(0.0, -gap, 0.0), p1=(L, -gap, 0.0), N=N, kobs=0.0, obj_scale=0.5)])
    rows[:, D.SC_KCOL], rows[:, D.SC_RCOL], rows[:, D.SC_SCOL] = 10.0, 10.0, 1.0 / N
    rows[0, D.SC_PMASK], rows[1, D.SC_PMASK] = 2, 1
    T = (N - 1) * H0
    R = max(0.06 * L, 1.2)
    trk = line_track((0.5 * L, 0.9 * R), (0.0, -3.0), GROUP_T_START + 0.5 * T, T, R)
    return rows, [M.straight_guess(r, N) for r in rows], [trk]


# ---- the independent arbiter: tests/golden/nlp_keepout_moving_slsqp.npz (tests/golden/make_nlp_keepout_moving_golden.py) -----------------
ARB_N = K.ARB_N
ARB_KINDS = ('cross', 'overtake')
ARB_T_START = 1.0


def arbiter_problem(N, kind):
    """A case of the golden file: the leg, row, start and disc (R = 3 % of the leg, its centre 0.3 R off the leg's axis at mid-leg; at 5
    nodes mirrored) of nlp_keepout_ref.arbiter_problem(N, False), with the disc MOVING, node 0 at ARB_T_START.  'cross': it crosses the
    leg at 2 m/s TOWARDS the side its centre is off to, and is at the static case's centre at mid-time: the near side of the static case
    stays the near side at every node, so the central path and SLSQP, which both start from the start rule's side, pass on the same one
    (nlp_keepout_ref.arbiter_problem's note).  'overtake': it runs along the leg 0.3 R off the axis, from 1.5 R behind p0 to 1.5 R
    beyond p1, and passes the aircraft.  -> oracle Problem, scenario row, W0, [track]."""
    pb, row, W0, discs = K.arbiter_problem(N, False)
    T = (N - 1) * pb.h
    tm = ARB_T_START + 0.5 * T
    c, R = discs[0, :2], float(discs[0, 2])
    mid = 0.5 * (pb.p0[:2] + pb.p1[:2]); leg = pb.p1[:2] - pb.p0[:2]; ll = float(np.hypot(*leg)); ax = leg / ll
    off = c - mid; side = off / float(np.hypot(*off))
    trk = line_track(c, 2.0 * side, tm, T, R) if kind == 'cross' else line_track(c, (ll + 3.0 * R) / T * ax, tm, T, R)
    return pb, row, W0, [trk]
