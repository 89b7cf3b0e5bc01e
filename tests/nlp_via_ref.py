"""CPU statement of the collocation problem through timed waypoints (include/d2d.h d2d_nlp_solve_via, d2d_nlp_solve_groups_via;
test infrastructure only).  Nothing new is solved here: a pin is a fixed variable, and the statements take their fixed set from
pb.lo == pb.hi per (node, component) -- oracle.nlp.solve, nlp_wind_ref.solve, nlp_groups_pairs_ref.solve_groups, all unchanged.
pin() writes the pins of a d2d_via_points table into an oracle Problem.

A TABLE is what the device reads: rows (node, mask, x, y, psi), mask bit 0 / 1 / 2 = x / y / psi pinned, a row of mask 0 absent.

The catalogue (chosen and measured on the CPU with these statements alone, before any GPU run; N = 61, h = 0.1, p0 = (0, 0, 0), the
row of nlp_moving_ref.row() without a disc: vsp 12, kv 70, kphi 1, obj_scale 1, phi within +-30 deg, v in 9 .. 14 m/s; guess():
piecewise linear through the pins that hold both x and y).  Still air, p1 = (72, 0, 0) -- status, Newton steps, cost:
  point       node 30: (36, 8)                       CONVERGED  39   7.850690
  heading     node 30: (36, 8), psi = 0              CONVERGED  39   7.871564
  slalom      node 20: (24, 3); node 40: (48, -3)    CONVERGED  42   4.404342
  adjacent    node 30: (36, 5); node 31: (37.2, 5)   CONVERGED  45   1.148710
  xonly       node 30: x = 34; node 45: y = 3        CONVERGED  71  22.759236
  yonly       node 30: y = 4                         CONVERGED  55   0.462687
  psionly     node 30: psi = 0.3                     CONVERGED  41   0.215452
  first       node 1: (1.2, 0)                       CONVERGED  12   0
  last        node 59: (70.8, 0)                     CONVERGED  12   0
  box         point, x in [-5, 80], y in [-2, 9]     CONVERGED  41   7.850690
  unreachable node 30: (36, 40)                      STALLED    41   feas 5.844
The gust of nlp_wind_ref.fields() from t_start 2.5 on the 48 m leg, p1 = (48, 0, 0):
  gust-point   node 30: (24, 5)                      CONVERGED  55   7.210691
  gust-heading node 30: (24, 5), psi = 0             CONVERGED  62   7.610249
  gust-xonly   node 30: x = 23; node 45: y = 2       CONVERGED  65  22.437156
  gust-yonly   node 30: y = 3                        CONVERGED  57   0.017052
  gust-psionly node 30: psi = 0.2                    CONVERGED  57   0.030213
Under a 1e-9 perturbation of the guess every status and every step count but gust-point's (60) is the same, and the plan moves by
<= 4e-9 (tests/test_via_cpu.py holds the statuses).  Dropped: an x pin alone on the straight line (x = 34 .. 38 at node 30, or
23 .. 24.5 in the gust).  The straight guess is mirror-symmetric there, the statement leaves it to one side or the other by rounding
alone, and the perturbed run ends 2.7 .. 3.8 m away after 3 .. 6 times the steps; the y pin at node 45 decides the side.
Other shapes (shapes(); legs of 1.2 m per node along x, steps and cost of the statement):
  n3    node 1: (1.2, 0) -- no free position left                                  12  0
  n4    nodes 1, 2 on the line -- two neighbouring fixed nodes, E between them 0   12  0
  n7    node 3: (3.6, 0.1)                                                         33  0.120518
  n66   nodes 63, 64: (75.6, 0.03), (76.8, 0) -- with the end node 65 three fixed nodes across the 64-lane chunk boundary; node 64 has
        to stand on the line: backward Euler and psi_65 = 0 give y_65 = y_64 ((76.8, 0.02) is STALLED, feas 0.2)     27  0.001452
  n121  (36, 5), (72, -5), (108, 5) at nodes 30 / 60 / 90                          47  9.591824
  mid3  N = 61, nodes 29, 30, 31: (34.8, 5), (36, 5), (37.2, 5) -- where the twisted serial recursion meets (m = N / 2 = 30)   45  1.207493
  n130  nodes 64, 65: (76.8, 6), (78, 6) -- cyclic-reduction records in global memory                               33  0.104135"""
import numpy as np

import nlp_moving_ref as M
import nlp_wind_ref as R
from oracle import nlp

N_NODES, H = M.N_NODES, M.H
X, Y, PSI = 1, 2, 4
XY, XYPSI = 3, 7


def rows_of(*pins):
    """pins (node, {0: x, 1: y, 2: psi}) -> table rows (node, mask, x, y, psi)."""
    out = []
    for node, vals in pins:
        r = [float(node), float(sum(1 << c for c in vals)), 0.0, 0.0, 0.0]
        for c, v in vals.items():
            r[2 + c] = float(v)
        out.append(r)
    return np.array(out, dtype=np.float64).reshape(-1, 5)


def table(rows, n_via=None):
    """rows padded with absent rows (mask 0) to n_via -> (n_via, 5)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    n_via = len(rows) if n_via is None else n_via
    out = np.zeros((n_via, 5))
    out[:len(rows)] = rows
    return out


def tables(per_problem):
    """One table per problem, padded to the longest -> (G, n_via, 5)."""
    n = max(1, max(len(np.asarray(t).reshape(-1, 5)) for t in per_problem))
    return np.stack([table(t, n) for t in per_problem])


def pin(pb, tab):
    """pb with lo == hi == value on every pinned (node, component) of the table; rows of mask 0 are absent."""
    for node, mask, *val in np.asarray(tab, dtype=np.float64).reshape(-1, 5):
        for c in range(3):
            if (int(mask) >> c) & 1:
                pb.lo[int(node), c] = pb.hi[int(node), c] = val[c]
    return pb


def guess(r, tab, N=N_NODES):
    """(N, 5): piecewise linear through the row's end points and the table's rows that pin both x and y, psi along each leg, phi = 0,
    v = vsp.  Without such rows: nlp_moving_ref.straight_guess."""
    import d2dhip as D
    from d2d.opty_utils import via_guess, Waypoint
    wps = [Waypoint(node * H, x, y) for node, mask, x, y, _ in np.asarray(tab, dtype=np.float64).reshape(-1, 5) if (int(mask) & 3) == 3]
    if not wps:
        return M.straight_guess(r, N)
    return np.stack(via_guess(r[D.SC_X0:D.SC_X0 + 3], r[D.SC_X1:D.SC_X1 + 3], wps, 0.0, H, N, r[D.SC_VSP]), 1)


def problem(r, tab, N=N_NODES, moving=(), t_start=0.0):
    return pin(M.problem(r, list(moving), t_start, N=N), tab)


def solve(pb, W0, field=None, t_start=0.0, **kw):
    return M.solve(pb, W0, field, t_start, **kw)


def boxed_row(r, x_box, y_box):
    import d2dhip as D
    r = r.copy()
    r[D.SC_XMIN], r[D.SC_XMAX] = x_box
    r[D.SC_YMIN], r[D.SC_YMAX] = y_box
    return r


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------
def catalogue(wind='const'):
    """name -> (row, table) at N = 61."""
    if wind == 'const':
        r = M.row(1, p1=(M.LEG, 0.0, 0.0), kobs=0.0)
        return {
            'point': (r, rows_of((30, {0: 36.0, 1: 8.0}))),
            'heading': (r, rows_of((30, {0: 36.0, 1: 8.0, 2: 0.0}))),
            'slalom': (r, rows_of((20, {0: 24.0, 1: 3.0}), (40, {0: 48.0, 1: -3.0}))),
            'adjacent': (r, rows_of((30, {0: 36.0, 1: 5.0}), (31, {0: 37.2, 1: 5.0}))),
            'xonly': (r, rows_of((30, {0: 34.0}), (45, {1: 3.0}))),
            'yonly': (r, rows_of((30, {1: 4.0}))),
            'psionly': (r, rows_of((30, {2: 0.3}))),
            'first': (r, rows_of((1, {0: 1.2, 1: 0.0}))),
            'last': (r, rows_of((59, {0: 70.8, 1: 0.0}))),
            'box': (boxed_row(r, (-5.0, 80.0), (-2.0, 9.0)), rows_of((30, {0: 36.0, 1: 8.0}))),
        }
    r = M.row(1, p1=(M.LEG_GUST, 0.0, 0.0), kobs=0.0)
    return {
        'gust-point': (r, rows_of((30, {0: 24.0, 1: 5.0}))),
        'gust-heading': (r, rows_of((30, {0: 24.0, 1: 5.0, 2: 0.0}))),
        'gust-xonly': (r, rows_of((30, {0: 23.0}), (45, {1: 2.0}))),
        'gust-yonly': (r, rows_of((30, {1: 3.0}))),
        'gust-psionly': (r, rows_of((30, {2: 0.2}))),
    }


UNREACHABLE = rows_of((30, {0: 36.0, 1: 40.0}))      # STALLED on the statement, feas 5.8
GUST_T_START = M.GUST_T_START

# name -> cost of the statement from guess(), as measured above (tests/test_via_cpu.py compares to 5e-6)
COSTS = {'point': 7.850690, 'heading': 7.871564, 'slalom': 4.404342, 'adjacent': 1.148710, 'xonly': 22.759236, 'yonly': 0.462687,
         'psionly': 0.215452, 'first': 0.0, 'last': 0.0, 'box': 7.850690, 'gust-point': 7.210691, 'gust-heading': 7.610249,
         'gust-xonly': 22.437156, 'gust-yonly': 0.017052, 'gust-psionly': 0.030213}
# name -> (Newton steps, cost) of the shapes() from guess(), as listed above (tests/test_via_cpu.py: steps equal, cost to 5e-6)
SHAPES_MEASURED = {'n3': (12, 0.0), 'n4': (12, 0.0), 'n7': (33, 0.120518), 'n66': (27, 0.001452), 'n121': (47, 9.591824),
                   'mid3': (45, 1.207493), 'n130': (33, 0.104135)}
# name -> Newton steps of the catalogue from guess() (the unreachable point: 41, STALLED)
STEPS = {'point': 39, 'heading': 39, 'slalom': 42, 'adjacent': 45, 'xonly': 71, 'yonly': 55, 'psionly': 41, 'first': 12, 'last': 12, 'box': 41,
         'gust-point': 55, 'gust-heading': 62, 'gust-xonly': 65, 'gust-yonly': 57, 'gust-psionly': 57}


def shapes():
    """name -> (N, row, table): the node counts at which the kernel takes another path."""
    def leg(N):
        return M.row(1, p1=(1.2 * (N - 1), 0.0, 0.0), N=N, kobs=0.0)
    return {
        'n3': (3, leg(3), rows_of((1, {0: 1.2, 1: 0.0}))),
        'n4': (4, leg(4), rows_of((1, {0: 1.2, 1: 0.0}), (2, {0: 2.4, 1: 0.0}))),
        'n7': (7, leg(7), rows_of((3, {0: 3.6, 1: 0.1}))),
        'n66': (66, leg(66), rows_of((63, {0: 75.6, 1: 0.03}), (64, {0: 76.8, 1: 0.0}))),
        'n121': (121, leg(121), rows_of((30, {0: 36.0, 1: 5.0}), (60, {0: 72.0, 1: -5.0}), (90, {0: 108.0, 1: 5.0}))),
        'mid3': (61, leg(61), rows_of((29, {0: 34.8, 1: 5.0}), (30, {0: 36.0, 1: 5.0}), (31, {0: 37.2, 1: 5.0}))),
        'n130': (130, leg(130), rows_of((64, {0: 76.8, 1: 6.0}), (65, {0: 78.0, 1: 6.0}))),
    }


# ---- groups: the first crossing of nlp_groups_pairs_ref with a pin on aircraft 0 and on aircraft 2 ------------------------------------
def group_pins(rows, offsets={0: 2.0, 2: -2.0}, node=30):
    """One (x, y) pin per aircraft of `offsets`: the middle of its straight leg moved sideways (to its left) by the offset, at `node`.
    -> one table per aircraft (absent rows for the others)."""
    import d2dhip as D
    out = []
    for a, r in enumerate(rows):
        if a not in offsets:
            out.append(np.zeros((1, 5)))
            continue
        p0, p1 = r[D.SC_X0:D.SC_X0 + 2], r[D.SC_X1:D.SC_X1 + 2]
        d = (p1 - p0) / np.hypot(*(p1 - p0))
        c = p0 + (p1 - p0) * node / (N_NODES - 1) + offsets[a] * np.array([-d[1], d[0]])
        out.append(rows_of((node, {0: c[0], 1: c[1]})))
    return out
