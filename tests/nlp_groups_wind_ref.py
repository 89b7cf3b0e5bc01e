"""CPU statement of the multi-aircraft collocation problem in a wind field (include/d2d.h d2d_nlp_solve_groups_wind; test
infrastructure only): block Gauss-Seidel over tests/nlp_wind_ref.py solve().

  sweep 0      every aircraft of the scenario solved uncoupled (no partner), from its guess
  sweeps 1..   aircraft 0, then aircraft 1, each a full solve from its current nodes with pb.partner = the other's frozen (x, y)
               (oracle.nlp._obst_terms carries the partner into nlp_wind_ref._normal_equations and into cost / objective), until
               neither moved by more than tol (largest |dx|, |dy| over the nodes) in a sweep, or max_sweeps; a pair that has not
               settled reports status 2 (D2D_ST_MAXITER)

`inner` is the solver of one aircraft: nlp_wind_ref.solve in a field (the default, through FieldProblem), or oracle.nlp.solve in the
constant wind of the Problems -- the same alternation, which is how the statement is tied to the oracle in a uniform field.

The scenarios of tests/test_gpu_mission_wind.py (group_scenarios) were chosen here, on the CPU, by this statement alone; what was
tried and dropped is in that function's docstring.
"""
import numpy as np

import nlp_wind_ref as R
from oracle import nlp

N_AC, N_NODES, H = 4, 61, 0.1                    # trap_4 as src/11_full_sim_case1.py drives it: 4 aircraft, hz = 10, t1 = 6 s
RCOL, KCOL = 10.0, 10.0                          # CostComposit(kvel=70, kbank=1, kcol=10, rcol=10), obj_scale = 1


def solve_groups(pbs, W0s, inner, max_sweeps=12, tol=1e-7):
    """pbs: the aircraft of ONE scenario (oracle Problems; 0 and 1 coupled when pbs[0].kcol > 0), W0s their guesses (N, 5);
    inner(a, pb, W0) -> (W, info).  Returns Ws, infos (of each aircraft's last solve; info['inner'] summed over its solves),
    sweeps, moved."""
    n = len(pbs)
    for pb in pbs:
        pb.partner = None
    Ws, infos = [], []
    for a in range(n):
        W, info = inner(a, pbs[a], W0s[a])
        Ws.append(W); infos.append(info)
    total = [info['inner'] for info in infos]
    sweep, moved = 0, 0.0
    if n >= 2 and pbs[0].kcol > 0.0:
        for sweep in range(1, max_sweeps + 1):
            mv = [0.0, 0.0]
            for turn in (0, 1):
                pbs[turn].partner = Ws[1 - turn][:, :2].copy()
                Wn, info = inner(turn, pbs[turn], Ws[turn])
                mv[turn] = float(np.abs(Wn[:, :2] - Ws[turn][:, :2]).max())
                total[turn] += info['inner']
                Ws[turn], infos[turn] = Wn, info
            moved = max(mv)
            if moved <= tol:
                break
        if moved > tol:
            for a in (0, 1):
                if infos[a]['status'] == 1:
                    infos[a] = dict(infos[a], status=2)
    for a in range(n):
        infos[a] = dict(infos[a], inner=total[a])
    return Ws, infos, sweep, moved


def in_field(field, t_start, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX):
    """inner solver of solve_groups: nlp_wind_ref.solve in `field`, node 0 at t_start."""
    return lambda a, pb, W0: R.solve(R.FieldProblem(pb, field, t_start), W0, inner_max=inner_max, outer_max=outer_max)


def in_constant_wind(inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX):
    """inner solver of solve_groups: oracle.nlp.solve in each Problem's own constant wind."""
    return lambda a, pb, W0: nlp.solve(pb, W0, inner_max=inner_max, outer_max=outer_max)


def group_rows(p0s, p1s, wind=(0.0, 0.0)):
    """d2dhip scenario rows (n_ac, SCEN_STRIDE) of one trap_4-like scenario, as opty.direct_collocation.Problem._rows lowers
    multi_opt_planner.trap_4: s = obj_scale / N / n_ac, the collision columns on rows 0 and 1 with scale obj_scale / N."""
    import d2dhip as D
    n = len(p0s)
    rows = np.zeros((n, D.SCEN_STRIDE))
    for a in range(n):
        r = rows[a]
        r[D.SC_X0:D.SC_X0 + 3] = p0s[a][:3]; r[D.SC_X1:D.SC_X1 + 3] = p1s[a][:3]
        r[D.SC_VSP], r[D.SC_KV], r[D.SC_KPHI], r[D.SC_S] = 12.0, 70.0, 1.0, 1.0 / N_NODES / n
        r[D.SC_WX], r[D.SC_WY] = -wind[0], -wind[1]
        r[D.SC_PHIMAX], r[D.SC_VMIN], r[D.SC_VMAX] = np.deg2rad(40.0), 9.0, 15.0
        r[D.SC_XMIN], r[D.SC_XMAX], r[D.SC_YMIN], r[D.SC_YMAX] = -150.0, 150.0, -150.0, 150.0
    rows[:2, D.SC_KCOL], rows[:2, D.SC_RCOL], rows[:2, D.SC_SCOL] = KCOL, RCOL, 1.0 / N_NODES
    return rows


def problems_of(rows):
    """The oracle Problems the rows describe (oracle.nlp.problem_from_row: what the kernel reads from them)."""
    return [nlp.problem_from_row(r, N_NODES, H) for r in rows]


def guesses(rows):
    """The reference's 'tri' guess of every row, (N, 5) each."""
    import d2dhip as D
    from oracle import costs as C
    out = []
    for r in rows:
        p0 = tuple(r[D.SC_X0:D.SC_X0 + 3]) + (0.0, 12.0); p1 = tuple(r[D.SC_X1:D.SC_X1 + 3]) + (0.0, 12.0)
        out.append(nlp.from_free(C.single_guess('tri', p0, p1, 12.0, (N_NODES - 1) * H, N_NODES), N_NODES))
    return out


# per field: the start time of each of the three scenarios (the gust is unsteady: a different start time per scenario)
T_STARTS = {'shear': (0.0, 0.0, 0.0), 'vortex': (0.0, 0.0, 0.0), 'gust': (0.0, 2.5, 6.0)}


# per scenario: distance of aircraft 1 below aircraft 0 at the start and at the end of the leg, the leg's dx and dy (metres)
SPEC = ((9.0, 9.5, 56.0, 4.0), (9.5, 9.0, 52.0, -6.0), (9.2, 9.6, 54.0, 8.0))


def group_scenarios(spec=SPEC):
    """Three trap_4-like scenarios (4 aircraft, 61 nodes, h = 0.1: hz = 10, t1 = 6 s; kvel = 70, kbank = 1, kcol = 10, rcol = 10,
    obj_scale = 1, phi within +-40 deg, v in 9 .. 15 m/s, positions in +-150 m) -> list of rows (4, SCEN_STRIDE).  Aircraft 0 and 1
    fly side by side 9 .. 9.6 m apart, inside rcol = 10 m, so the collision term acts along the whole leg (the uncoupled solutions come
    within 8.4 .. 9.3 m of each other in the three fields: tests/test_mission_wind_cpu.py asserts < rcol); aircraft 2 and 3 fly
    uncoupled legs of their own with a heading change.  The legs are 52 .. 56 m in 6 s: the fields blow 2 .. 5 m/s against +x (the model
    ADDS the field to the residual), which puts the airspeed near vsp = 12 m/s.
    Chosen on the CPU with this statement alone, in the three fields of nlp_wind_ref.fields() at T_STARTS: every inner solve converges,
    the pair settles in 5 .. 10 sweeps (12 allowed) at tol 1e-7 (last moves 2e-9 .. 4e-8), and under a 1e-9 perturbation of the guess
    the sweep counts do not change and the Newton-step counts of the pair move by at most 1 (an uncoupled aircraft's by 10 once).
    Tried and dropped: the same lay-out with the pair 5 .. 8 m apart and legs of 66 .. 70 m -- the legs then need 14 .. 16 m/s of
    airspeed against the shear and the gust (costs of 25 .. 100), the positions are flat directions of such a cost, and the alternation
    had not settled after 12 sweeps in seven of the nine cases (last moves 1e-7 .. 2e-6; Newton-step counts 780 against 624 under the
    perturbation); the pair 8 .. 8.6 m apart on the legs below -- one case of nine (gust, scenario 2) not settled after 12 sweeps;
    the pair 9.5 .. 9.8 m apart on legs of 48 .. 52 m -- one case (shear, scenario 0) not settled."""
    out = []
    for k, (gap0, gap1, dx, dy) in enumerate(spec):
        x0, y0 = -40.0 + 5.0 * k, 30.0 - 20.0 * k
        p0s = [(x0, y0, 0.0), (x0 + 1.0, y0 - gap0, 0.0), (x0 + 5.0, y0 - 45.0, 0.15), (x0 - 5.0, y0 - 70.0, -0.1)]
        p1s = [(x0 + dx, y0 + dy, 0.0), (x0 + 1.0 + dx, y0 + dy - gap1, 0.0), (x0 + 5.0 + dx, y0 - 45.0 + 8.0, -0.1),
               (x0 - 5.0 + dx, y0 - 70.0 - 5.0, 0.0)]
        out.append(group_rows(p0s, p1s))
    return out


# ---- the mission of tests/test_gpu_mission_wind.py (also timed by tools/bench_nlp_wind.py) ---------------------------------------
def mission_wind(t, x, y):
    """An unsteady field over the mission's own time span: the head wind wx grows linearly by 0.005 m/s per second from t = 100 s on
    (the spline clamps time outside its grid: before 100 s phase 1 flies the constant (1, 0)); uniform in space and without a cross
    component, because phase 1 ends when every aircraft passes its pose X1_f within 0.5 deg of heading 0, which a cross wind of
    0.13 m/s at 15 m/s already spends (tried first: a bump in wx with a cross component -0.5 a sin(y / 50) -- two of the three
    formations never ended phase 1; then this field growing by 0.02 m/s per second -- the formation that starts with a heading offset
    never ended it).  Two start times one phase-1 row (0.05 s) apart see winds that differ by 2.5e-4 m/s: a plan checked at another
    formation's start time misses its equalities by 2.5e-4 per row of difference.  (Fields that vary in space are
    the business of the solver's own tests above; this one is about the times handed from phase to phase.)"""
    a = 0.005 * (t - 100.0)
    return 1.0 + a + 0.0 * x, 0.0 * x + 0.0 * y


def mission_field():
    """mission_wind as a SplineWindField on the box of nlp_wind_ref.fields(), sample times 100 .. 210 s every 2 s (a cubic B-spline
    reproduces what is linear in t)."""
    import wind_ref as WR
    return WR.spline_of(mission_wind, t=np.arange(100.0, 210.5, 2.0))


def mission_inputs():
    """Three formations of four aircraft on the circles of src/11_full_sim_case1.py that start phase 1 from different states (so that
    they end it at different rows): n_ac, c (4, 2), X1_f, X2_f (4, 5), X0 (3, 4, 5), ref3 = (time_3, x3, y3) a closed loop of 120 steps."""
    n_ac = 4
    c = np.array([[0, -20], [25, -20], [25, -100], [0, -100]], float)
    X1_f = np.array(((0, 40, 0, 0, 12), (25, 40, 0, 0, 12), (25, -40, 0, 0, 12), (0, -40, 0, 0, 12)), float)
    X2_f = np.array(((75, 40, 0, 0, 12), (100, 40, 0, 0, 12), (100, -40, 0, 0, 12), (75, -40, 0, 0, 12)), float)
    X0B = np.tile(np.array([20, 30, -np.pi / 2, 0, 10.0]), (3, n_ac, 1))            # (src/11_full_sim_case1.py:113)
    X0B[1, :, :2] += (6.0, -4.0); X0B[2, :, :2] += (-8.0, 5.0); X0B[2, :, 2] += 0.3
    T3 = 120
    th = np.linspace(0, 2 * np.pi, T3)
    time_3 = np.arange(T3) * 0.1
    x3 = X2_f[None, :, 0] + 30 * np.sin(th)[:, None]; y3 = X2_f[None, :, 1] + 30 * (1 - np.cos(th))[:, None]
    return n_ac, c, X1_f, X2_f, X0B, (time_3, x3, y3)


def mission_t_end(stop_rows, n_rows, t_step, t_opt, time_3, passes):
    """t_sim_end that leaves room for exactly `passes` repetitions of phase 3 (the loop count follows the slowest formation)."""
    return float((np.minimum(stop_rows, n_rows).max() - 1) * t_step + t_opt + passes * time_3[-1] - 1e-6)
