"""CPU statement of the collocation problem around moving obstacles (include/d2d.h d2d_nlp_solve_moving,
d2d_nlp_solve_groups_moving; test infrastructure only).  Nothing new is solved here: a moving disc is a CostObstacle disc whose
centre at node i is the track at t_start + i h, and oracle.nlp._obst_terms broadcasts over array-valued centres, so

  single problems   oracle.nlp.Problem(obstacles=[(cx, cy, r)]) with cx, cy arrays (N,) from MovingObstacle.at, solved by
                    oracle.nlp.solve (constant wind) or nlp_wind_ref.solve (a field) on the SAME Problem;
  groups            nlp_groups_pairs_ref.solve_groups over such Problems: the discs' terms come before the partners', as on the device.

The discs of a Problem share one kind (oracle.nlp.Problem.obs_kind), which is all the catalogue needs.
"""
import numpy as np

import nlp_groups_pairs_ref as P
import nlp_wind_ref as R
from d2d.opty_utils import MovingObstacle
from oracle import nlp

N_NODES, H = 61, 0.1
KOBS = {1: 10.0, 0: 0.5}                         # the catalogue's obstacle weight per CostObstacle kind
LEG, LEG_GUST = 72.0, 48.0                       # leg length: 12 m/s over the ground in still air; 8 m/s against the gust's 3 .. 5 m/s
P0, P1 = (0.0, 0.0, 0.0), (LEG, 0.0, 0.0)
T_END = 20.0                                     # the catalogue's tracks are straight lines over [0, T_END] s


def node_times(t_start, N=N_NODES, h=H):
    return t_start + np.arange(N) * h


def row(kind=1, p0=P0, p1=P1, N=N_NODES, wind=(0.0, 0.0), kobs=None, obj_scale=1.0, kv=70.0, kphi=1.0):
    """The d2dhip scenario row of the catalogue's common settings: vsp = 12, kv = 70, kphi = 1, kobs = 10 (kind 1) or 0.5 (kind 0),
    obj_scale = 1, and oracle.nlp.Problem's default bounds: phi within +-30 deg, v in 9 .. 14 m/s, no position box."""
    import d2dhip as D
    r = np.zeros(D.SCEN_STRIDE)
    r[D.SC_X0:D.SC_X0 + 3] = p0[:3]; r[D.SC_X1:D.SC_X1 + 3] = p1[:3]
    r[D.SC_VSP], r[D.SC_KV], r[D.SC_KPHI], r[D.SC_S] = 12.0, kv, kphi, obj_scale / N
    r[D.SC_KOBS] = KOBS[kind] if kobs is None else kobs
    r[D.SC_WX], r[D.SC_WY] = -wind[0], -wind[1]
    r[D.SC_PHIMAX], r[D.SC_VMIN], r[D.SC_VMAX] = np.deg2rad(30.0), 9.0, 14.0
    return r


def with_moving(pb, moving, t_start):
    """pb with the moving discs appended to its obstacles as array-valued centres at pb's node times.  Discs with r <= 0 are absent."""
    live = [o for o in moving if o.r > 0.0]
    if live:
        kinds = {o.kind for o in live}
        assert len(kinds) == 1 and (not pb.obstacles or pb.obs_kind == live[0].kind), 'one CostObstacle kind per oracle Problem'
        pb.obs_kind = live[0].kind
        t = node_times(t_start, pb.N, pb.h)
        pb.obstacles = tuple(pb.obstacles) + tuple((o.at(t)[:, 0], o.at(t)[:, 1], o.r) for o in live)
    return pb


def problem(r, moving, t_start=0.0, N=N_NODES, h=H):
    """The oracle Problem of scenario row r around the moving discs, node i at t_start + i h."""
    return with_moving(nlp.problem_from_row(r, N, h), moving, t_start)


def straight_guess(r, N=N_NODES):
    """(N, 5): the straight line between the row's end points at vsp."""
    import d2dhip as D
    W = np.zeros((N, 5))
    W[:, 0] = np.linspace(r[D.SC_X0], r[D.SC_X1], N); W[:, 1] = np.linspace(r[D.SC_Y0], r[D.SC_Y1], N)
    W[:, 2] = np.linspace(r[D.SC_PSI0], r[D.SC_PSI1], N); W[:, 4] = r[D.SC_VSP]
    return W


def solve(pb, W0, field=None, t_start=0.0, **kw):
    """oracle.nlp.solve in pb's constant wind, or nlp_wind_ref.solve in `field` with node 0 at t_start; kw goes to the solver."""
    return nlp.solve(pb, W0, **kw) if field is None else R.solve(R.FieldProblem(pb, field, t_start), W0, **kw)


def solve_groups(rows, moving, W0s, field=None, t_start=0.0, max_sweeps=P.MAX_SWEEPS, N=N_NODES, h=H, **kw):
    """One scenario of len(rows) aircraft with the partner sets of the rows' SC_PMASK, every aircraft around the same moving discs;
    kw (inner_max, outer_max) goes to every solve."""
    pbs = [with_moving(nlp.problem_from_row(r, N, h), moving, t_start) for r in rows]
    inner = P.in_constant_wind(**kw) if field is None else P.in_field(field, t_start, **kw)
    return P.solve_groups(pbs, W0s, inner, P.masks_of(rows), max_sweeps=max_sweeps)


def tables(moving_per_problem, n_knot=None):
    """knots (G, n_mov, n_knot, 3) and disc (G, n_mov, 2) of a list of disc lists (the same count in each)."""
    from d2d.opty_utils import lower_moving
    n_knot = n_knot or max(len(o.t) for m in moving_per_problem for o in m)
    tabs = [lower_moving(m, n_knot) for m in moving_per_problem]
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


# ---- the catalogue (chosen on the CPU with this statement alone, before any GPU run) ------------------------------------------------
def crossing_disc(kind, t0=0.0, leg=LEG, r=8.0):
    """Crosses the leg from below at 10 m/s: on the track at mid-leg three seconds after t0, when the aircraft is there."""
    return MovingObstacle.linear((leg / 2, -28.0), (0.0, 10.0), r, t0=t0, t1=t0 + T_END, kind=kind)


def headon_disc(kind, t0=0.0, leg=LEG):
    """Comes down the leg at the aircraft's own ground speed, 1.5 m to its left, from 8 m behind the leg's end."""
    return MovingObstacle.linear((leg + 8.0, 1.5), (-leg / 6.0, 0.0), 8.0, t0=t0, t1=t0 + T_END, kind=kind)


def second_disc(kind, t0=0.0, leg=LEG):
    return MovingObstacle.linear((leg - 12.0, 20.0), (-6.0, -5.0), 6.0, t0=t0, t1=t0 + T_END, kind=kind)


def catalogue(kind, t0=0.0, leg=LEG):
    """name -> the moving discs of a starting scenario (N = 61, h = 0.1, p0 = (0, 0, 0), p1 = (leg, 0, 0), row(kind)); t0: the time the
    tracks are anchored at (the scenario's t_start: the encounter is the same whatever the clock reads).  With leg = 72 m:
      crossing  (36, -28 + 10 t), r = 8;  headon  (80 - 12 t, 1.5), r = 8;  two  crossing's disc and (60 - 6 t, 20 - 5 t), r = 6.
    From the straight-line guess all six (three scenarios x two kinds) end CONVERGED in still air with feas <= 6e-10, in 35 .. 37
    (kind 1) and 209 .. 230 (kind 0) Newton steps, lateral detours 4.4 .. 7.7 m, costs
      crossing 1.3708 / 7.8155,  headon 0.7802 / 3.1357,  two 1.3838 / 7.8155   (kind 1 / kind 0).
    In the unsteady gust of nlp_wind_ref.fields() (start time GUST_T_START) the 72 m leg cannot be flown -- the gust blows 3 .. 5 m/s
    against it and v_max is 14 m/s: the statement ends STALLED, feas 0.8 -- so the gust runs use leg = LEG_GUST = 48 m, the discs
    placed by the same rule.  There the kind-0 crossing disc has r = 5 m: at 8 m/s over the ground the aircraft stays under the
    r = 8 m disc's clipped exp(r^2 - d^2) for most of the leg -- the statement needed 585 .. 646 Newton steps (cost 42) and its step
    count moved by 150 under a 1e-9 perturbation of the guess (r = 6: 242 steps; r = 5: 119 / 118 steps, cost 3.59, detour 6.9 m).
    tests/test_moving_obstacles_cpu.py holds every status under that perturbation."""
    rc = 5.0 if (kind == 0 and leg != LEG) else 8.0
    return {'crossing': [crossing_disc(kind, t0, leg, rc)], 'headon': [headon_disc(kind, t0, leg)],
            'two': [crossing_disc(kind, t0, leg, rc), second_disc(kind, t0, leg)]}


GUST_T_START = 2.5                               # the start time of the catalogue's runs in the unsteady gust of nlp_wind_ref.fields()


def cases():
    """(wind, kind, name, leg, t_start) of the catalogue's twelve runs."""
    return [(w, kind, name, LEG if w == 'const' else LEG_GUST, 0.0 if w == 'const' else GUST_T_START)
            for w in ('const', 'gust') for kind in (1, 0) for name in ('crossing', 'headon', 'two')]


# ---- groups: two four-aircraft crossings of nlp_groups_pairs_ref with a disc through each -------------------------------------------
GROUP_KOBS = 10.0


def group_scenarios():
    """The first two scenarios of nlp_groups_pairs_ref.pair_scenarios() (all six pairs coupled, the rows' wind CONST_WIND) with the
    obstacle weight kobs = 10 in every row -> list of rows (4, SCEN_STRIDE)."""
    import d2dhip as D
    scs = P.pair_scenarios()[:2]
    for sc in scs:
        sc[:, D.SC_KOBS] = GROUP_KOBS
    return scs


def group_discs(t0s=(0.0, 0.0)):
    """One kind-1 disc of radius 6 m per scenario that crosses the formation's tracks near the middle of the legs about three seconds
    after the scenario's start: from the south at 8 m/s in scenario 0, from the north-east at (-4, -7) m/s in scenario 1."""
    return [[MovingObstacle.linear((-13.0, -26.0), (0.0, 8.0), 6.0, t0=t0s[0], t1=t0s[0] + T_END)],
            [MovingObstacle.linear((2.0, 12.0), (-4.0, -7.0), 6.0, t0=t0s[1], t1=t0s[1] + T_END)]]
