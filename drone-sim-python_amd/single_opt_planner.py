"""Mirror of src/single_opt_planner.py: the single-aircraft trajectory planner, solved on the
GPU.  Where the reference hands a direct-collocation NLP to opty/IPOPT
(src/single_opt_planner.py:62-71,124), this Planner fits a 6-segment C^3 degree-7 polynomial
to the same objective (flat outputs -> (psi, phi, v), the kinematic constraints hold
identically) with libd2dhip's batched Levenberg-Marquardt solver, then samples it at the
reference's nodes so that `solution`, `sol_*`, save/load keep the reference's layout."""
import os

import numpy as np

import d2dhip
import d2d.opty_utils as d2ou
import d2d.multiopty_utils as d2mou
import d2d.optyplan_scenarios as d2oscen

seed = None
# Which solver stands behind Planner.prob:
#   'fit' -- the batched polynomial fit (flat outputs, soft bounds; the north-star path)
#   'nlp' -- opty.direct_collocation.Problem on the GPU: the reference's own parameterisation (node values, backward-Euler
#            equalities, HARD bounds), built by the very call the reference makes (src/single_opt_planner.py:62-71)
#   'auto' (default) -- the fit first; if its plan overshoots a bound of the scenario (phi, v or the x / y box: the fit's bounds are
#            soft rows) by more than AUTO_TOL, the collocation problem is solved from that plan, so that what a script gets from
#            Planner(scen).run() never violates a bound IPOPT would have enforced; info['backend_used'] says which one answered.
#            A cost plug-in that lower_cost does not know (a user's own objective) goes straight to the collocation problem, which
#            calls its cost / cost_grad on the host (opty.direct_collocation, host objective): info['backend_used'] = 'nlp'.
#            So does a wind that varies in space and time (exp.wind a d2d.wind.SplineWindField; d2d_nlp_solve_wind): the fit's speed
#            and bank rows would depend on position through the field, and backend='fit' refuses it.
#            So do moving obstacles (exp.moving_obstacles, a list of d2d.opty_utils.MovingObstacle; d2d_nlp_solve_moving): the fit's
#            scenario row has no room for their tracks, and backend='fit' refuses them.
#            So do timed waypoints (exp.waypoints, a list of d2d.opty_utils.Waypoint; d2d_nlp_solve_via): the fit has no interior
#            conditions, and backend='fit' refuses them.
BACKEND = 'auto'
AUTO_TOL = 1e-6        # rad, m/s, m
N_SEG = 6
W_WAYPOINT = 0.02      # weight of the 'tri' waypoint rows (regulariser)
W_BOUND = 1.0          # weight of the soft phi / v bound rows

_plans = {}


def get_plan(K, duration, obj_scale_over_n, kv=5., kphi=1.):
    """Fit plans are cached per (K, duration, whitening metric): the basis block is shared by every trajectory that is
    fitted with the same node grid AND the same cost weights (the metric is the quadratic skeleton of the cost; a plan built
    for other weights spans the same space but is conditioned differently, so it is not reused)."""
    ctx = d2dhip.default_context()
    s = obj_scale_over_n
    wref = (W_WAYPOINT ** 2, s * max(kv, 1e-3), s * max(kphi, 1e-3) / 9.81 ** 2)
    key = (K, round(float(duration), 9)) + tuple(float(f'{w:.6e}') for w in wref)
    if key not in _plans:
        _plans[key] = d2dhip.FitPlan(ctx, N_SEG, K, duration, wref)
    return _plans[key]


MOVING_HOST_COST = ('moving obstacles together with a host objective (a cost plug-in without a kernel, d2d_nlp_solve_model) are not '
                    'supported: use one of the cost classes of d2d.opty_utils / d2d.multiopty_utils')


VIA_HOST_COST = ('timed waypoints together with a host objective (a cost plug-in without a kernel, d2d_nlp_solve_model) are not '
                 'supported: use one of the cost classes of d2d.opty_utils / d2d.multiopty_utils')


def check_waypoints(exp, backend, n_ac=None):
    """The scenario's timed waypoints (exp.waypoints, absent or empty: none), refused where they cannot be planned: backend='fit'.
    n_ac None: one list of d2d.opty_utils.Waypoint (single_opt_planner); else one list per aircraft (multi_opt_planner) -> a list of
    n_ac lists."""
    wps = getattr(exp, 'waypoints', None) or []
    if n_ac is None:
        wps = list(wps)
        if any(not isinstance(w, d2ou.Waypoint) for w in wps):
            raise ValueError('waypoints: a list of d2d.opty_utils.Waypoint')
        has = bool(wps)
    else:
        if any(isinstance(w, d2ou.Waypoint) for w in wps):
            raise ValueError(f'waypoints: one list of d2d.opty_utils.Waypoint per aircraft ({n_ac})')
        wps = [list(w or []) for w in wps] or [[] for _ in range(n_ac)]
        if len(wps) != n_ac or any(not isinstance(w, d2ou.Waypoint) for ws in wps for w in ws):
            raise ValueError(f'waypoints: one list of d2d.opty_utils.Waypoint per aircraft ({n_ac})')
        has = any(wps)
    if has and backend == 'fit':
        raise NotImplementedError("backend='fit' cannot plan through timed waypoints: the polynomial fit has no interior conditions.  "
                                  "backend='nlp' (or 'auto') solves the collocation problem through them")
    return wps if has else ([] if n_ac is None else [[] for _ in range(n_ac)])


def waypoint_constraints(ac, waypoints):
    """The instance constraints of one aircraft's waypoints: `x(t) - value` for every pinned component."""
    out = ()
    for w in waypoints:
        for sym, v in ((ac._sx, w.x), (ac._sy, w.y), (ac._spsi, w.psi)):
            if v is not None:
                out += (sym(w.t) - v,)
    return out


def check_moving(exp, backend):
    """The scenario's moving obstacles (exp.moving_obstacles, absent or empty: none) as a list, refused where they cannot be planned:
    backend='fit', more discs than d2dhip.MAX_MOV, a track with more knots than d2dhip.MOV_MAX_KNOT."""
    moving = list(getattr(exp, 'moving_obstacles', None) or [])
    if moving and backend == 'fit':
        raise NotImplementedError("backend='fit' cannot plan around moving obstacles: the fit's scenario row has no room for their "
                                  "tracks and its kernels no registers for their terms.  backend='nlp' (or 'auto') solves the "
                                  "collocation problem around them")
    d2ou.lower_moving(moving)
    return moving


def check_keep_out(exp, backend, moving=(), waypoints=(), t1_free=None):
    """The scenario's hard keep-out discs (exp.keep_out, a list of d2d.opty_utils.KeepOut and MovingKeepOut -- with one that moves the
    list plans through d2d_nlp_solve_keepout_moving; absent or empty: none) as a list, refused where
    they cannot be planned: backend='fit', more than d2dhip.MAX_KEEP, or together with moving obstacles, waypoints or t1_free."""
    keep = list(getattr(exp, 'keep_out', None) or [])
    if not keep:
        return keep
    if backend == 'fit':
        raise NotImplementedError("backend='fit' cannot hold a keep-out disc (keep_out): the polynomial fit has soft rows only.  "
                                  "backend='nlp' (or 'auto') solves the collocation problem with the discs as hard constraints")
    for name, given in (('moving obstacles (moving_obstacles)', bool(moving)), ('waypoints', bool(waypoints)), ('a free duration (t1_free)', t1_free is not None)):
        if given:
            raise NotImplementedError(f'keep_out together with {name} is not supported: hard discs are planned without soft moving '
                                      'discs, without pins, with a fixed step (d2d_nlp_solve_keepout, d2d_nlp_solve_keepout_moving)')
    if len(keep) > d2dhip.MAX_KEEP:
        raise NotImplementedError(f'at most {d2dhip.MAX_KEEP} keep-out discs per problem in this build ({len(keep)} given)')
    return keep


def check_fence(exp, backend, moving=(), waypoints=(), t1_free=None, keep=()):
    """The scenario's hard geofence (exp.fence, a d2d.opty_utils.GeoFence; absent or None: none), refused where it cannot be planned:
    backend='fit', or together with moving obstacles, waypoints, t1_free or a MovingKeepOut in keep_out."""
    fence = getattr(exp, 'fence', None)
    if fence is None:
        return None
    if backend == 'fit':
        raise NotImplementedError("backend='fit' cannot hold a geofence (fence): the polynomial fit has soft rows only.  "
                                  "backend='nlp' (or 'auto') solves the collocation problem with the edges as hard constraints")
    import d2d.opty_utils as d2ou
    for name, given in (('moving obstacles (moving_obstacles)', bool(moving)), ('waypoints', bool(waypoints)), ('a free duration (t1_free)', t1_free is not None),
                        ('a MovingKeepOut in keep_out', any(isinstance(k, d2ou.MovingKeepOut) for k in keep))):
        if given:
            raise NotImplementedError(f'fence together with {name} is not supported: a geofence is planned with static hard discs, without '
                                      'moving discs, without pins, with a fixed step (d2d_nlp_solve_fence)')
    d2ou.lower_fence(fence)                       # (a GeoFence or its rows: anything else is refused here)
    return fence


FENCE_HOST_COST = ('fence together with a host objective (a cost plug-in without a kernel, d2d_nlp_solve_model) is not supported: '
                   'use one of the cost classes of d2d.opty_utils')


def lowerable(cost):
    """True if lower_cost knows the plug-in (the fit and the lowered collocation kernel can express it)."""
    try:
        lower_cost(cost)
        return True
    except NotImplementedError:
        return False


def fit_cost(cost):
    """lower_cost for the polynomial fit: a plug-in it does not know is refused with the reason."""
    try:
        return lower_cost(cost)
    except NotImplementedError as e:
        raise NotImplementedError(f"{e}: backend='fit' cannot plan with it -- the polynomial fit works on the structured cost terms "
                                  "and has no form for a scalar objective; backend='nlp' or 'auto' solve it with its cost / "
                                  "cost_grad on the host") from None


class Lowered(tuple):
    """lower_cost's tuple of a cost with a duration term: the same nine entries, and the weight of the duration as the attribute
    `kdur` (duration_weight reads it; a plain tuple has none: 0)."""
    kdur = 0.0

    def __new__(cls, entries, kdur):
        self = super().__new__(cls, entries)
        self.kdur = float(kdur)
        return self


def duration_weight(lowered):
    """k of the term k * duration of a lowered cost (CostDuration, CostComposit(kdur=)); 0 for every other cost."""
    return float(getattr(lowered, 'kdur', 0.0))


KEEP_HOST_COST = ('keep_out together with a host objective (a cost plug-in without a kernel, d2d_nlp_solve_model) is not supported: '
                  'use one of the cost classes of d2d.opty_utils')
FREE_TIME_FIT = ("backend='fit' cannot plan with a free duration (t1_free): the polynomial fit's basis is built for one duration.  "
                 "backend='nlp' (or 'auto') solves the collocation problem with the time step as an unknown")


def _free_duration(exp, backend, attr):
    """The free duration (t1_lo, t1_hi) in seconds that the scenario carries as `attr` (t1_free or t1_window) -> None or the pair: its
    range check and the refusal of the fit backend, the same for either spelling."""
    tf = getattr(exp, attr, None)
    if tf is None:
        return None
    lo, hi = (float(v) for v in tf)
    if not (np.isfinite(lo) and np.isfinite(hi)) or not lo > exp.t0 or not lo < hi:
        raise ValueError(f'{attr} = ({lo}, {hi}): t0 < t1_lo < t1_hi required (t0 = {exp.t0})')
    if backend == 'fit':
        raise NotImplementedError(FREE_TIME_FIT.replace('t1_free', attr))
    return lo, hi


def check_free_time(exp, backend):
    """The scenario's optional t1_free = (t1_lo, t1_hi) in seconds -> None or the pair, refused where it cannot be planned."""
    return _free_duration(exp, backend, 't1_free')


def check_window(exp, backend, moving=(), waypoints=(), t1_free=None, field=None):
    """The scenario's optional t1_window = (t1_lo, t1_hi) in seconds: t1_free's free duration for a plan that ALSO holds static KeepOuts
    and a fence (t1_free keeps refusing them; without either the plan is t1_free's) -> None or the pair.  It takes t1_free's checks and
    is refused by name where it cannot be planned: beside t1_free, moving obstacles, waypoints, a MovingKeepOut, a wind field that
    varies in space and time, or backend='fit'."""
    tw = _free_duration(exp, backend, 't1_window')
    if tw is None:
        return None
    import d2d.opty_utils as d2ou
    for name, given in (('t1_free (one spelling of the free duration per scenario)', t1_free is not None),
                        ('moving obstacles (moving_obstacles)', bool(moving)), ('waypoints', bool(waypoints)),
                        ('a MovingKeepOut in keep_out', any(isinstance(k, d2ou.MovingKeepOut) for k in (getattr(exp, 'keep_out', None) or []))),
                        ('a wind field that varies in space and time (SplineWindField)', field is not None)):
        if given:
            raise NotImplementedError(f't1_window together with {name} is not supported: a free duration holds static hard discs and a '
                                      'geofence for one aircraft in a constant wind (d2d_nlp_solve_free_fence)')
    return tw


def lower_cost(cost):
    """Recognise the reference's cost plug-ins structurally -> (vsp, kv, kphi, kobs, obstacles, kcol, rcol,
    okind, bankmax[, pairs]): okind = bit mask of the obstacles of CostObstacle kind 0, bankmax = CostBank max mode.
    A collision term that selects anything but the reference's pair (0, 1) appends its `pairs` argument as a tenth entry
    (collision_pairs_of resolves it); the default keeps the nine entries.
    A cost with a duration term (CostDuration, CostComposit(kdur=)) returns the same entries as a Lowered, whose attribute kdur is
    the weight (duration_weight); every other cost returns the plain tuple it always did.
    Anything else has no kernel and raises (there is no CPU solver to fall back to)."""
    nan = float('nan')
    if isinstance(cost, d2ou.CostDuration):
        return Lowered((0., 0., 0., 0., (), nan, 0., 0, 0), cost.k)
    if isinstance(cost, d2ou.CostAirVel):
        return cost.vsp, 1., 0., 0., (), nan, 0., 0, 0
    if isinstance(cost, d2ou.CostBank):
        return 0., 0., 1., 0., (), nan, 0., 0, 0 if cost.use_mean else 1
    if isinstance(cost, (d2ou.CostInput, d2mou.CostInput)):
        return cost.vsp, cost.kv, cost.kphi, 0., (), nan, 0., 0, 0
    if isinstance(cost, d2mou.CostNull):
        return 0., 0., 0., 0., (), nan, 0., 0, 0
    if isinstance(cost, (d2ou.CostObstacle, d2mou.CostObstacle)):          # one disc on its own (07_multioptyplan exp_3)
        return 0., 0., 0., 1., ((cost.c[0], cost.c[1], cost.r),), nan, 0., 1 if cost.kind == 0 else 0, 0
    if isinstance(cost, (d2ou.CostObstacles, d2mou.CostObstacles)):
        obss = tuple((o.c[0], o.c[1], o.r) for o in cost.obss)
        return 0., 0., 0., 1., obss, nan, 0., sum(1 << i for i, o in enumerate(cost.obss) if o.kind == 0), 0
    if isinstance(cost, d2mou.CostCollision):                              # the collision term on its own
        return (0., 0., 0., 0., (), 1., cost.r, 0, 0) + (() if cost.pairs is None else (cost.pairs,))
    if isinstance(cost, d2ou.CostComposit):
        obss = [(o.c[0], o.c[1], o.r) for o in cost.cobs.obss] if hasattr(cost, 'cobs') else []
        okind = sum(1 << i for i, o in enumerate(cost.cobs.obss) if o.kind == 0) if obss else 0
        low = cost.cvel.vsp, cost.kvel, cost.kbank, cost.kobs, tuple(obss), nan, 0., okind, 0 if cost.cbank.use_mean else 1
        return Lowered(low, cost.kdur) if hasattr(cost, 'cdur') else low
    if isinstance(cost, d2mou.CostComposit):
        obss = ()
        kobs = 0.
        okind = 0
        if not np.isnan(cost.kobs):
            obss = tuple((o[0], o[1], o[2]) for o in cost.obss)
            kobs = cost.kobs
            okind = ((1 << len(obss)) - 1) if cost.obs_kind == 0 else 0
        return (cost.vsp, cost.kvel, cost.kbank, kobs, obss, cost.kcol, cost.rcol, okind, 0) + (
            () if getattr(cost, 'col_pairs', None) is None else (cost.col_pairs,))
    raise NotImplementedError(f'cost plug-in {type(cost).__name__} has no HIP lowering')


def collision_pairs_of(lowered, n):
    """The pairs a lowered cost couples among n aircraft, or None for the reference's pair (0, 1) (lower_cost's nine entries).
    ValueError for malformed pairs (d2d.multiopty_utils.collision_pairs)."""
    if len(lowered) <= 9:
        return None
    return d2mou.collision_pairs(lowered[9], n)


def scen_row(p0, p1, vref, lowered, s, wind, phi_c, v_c, go_left=-1., x_c=None, y_c=None):
    """One d2dhip scenario row.  The reference's symbolic model adds the wind with the opposite
    sign to the plant (src/d2d/opty_utils.py:42-44 vs src/d2d/dynamic.py:18-19); the planner keeps
    that convention, hence -w."""
    vsp, kv, kphi, kobs, obss = lowered[:5]
    okind, bankmax = lowered[7], lowered[8]
    if len(obss) > d2dhip.MAX_OBS:
        raise NotImplementedError(f'at most {d2dhip.MAX_OBS} static obstacles per trajectory in this build')
    r = np.zeros(d2dhip.SCEN_STRIDE)
    r[d2dhip.SC_X0], r[d2dhip.SC_Y0], r[d2dhip.SC_PSI0] = p0[0], p0[1], p0[2]
    r[d2dhip.SC_X1], r[d2dhip.SC_Y1], r[d2dhip.SC_PSI1] = p1[0], p1[1], p1[2]
    r[d2dhip.SC_VREF], r[d2dhip.SC_VSP] = vref, vsp
    r[d2dhip.SC_KV], r[d2dhip.SC_KPHI], r[d2dhip.SC_KOBS], r[d2dhip.SC_S] = kv, kphi, kobs, s
    r[d2dhip.SC_WWP], r[d2dhip.SC_WBND], r[d2dhip.SC_GOLEFT] = W_WAYPOINT, W_BOUND, go_left
    r[d2dhip.SC_WX], r[d2dhip.SC_WY] = -wind[0], -wind[1]
    for i, o in enumerate(obss):
        c = d2dhip.obs_col(i)
        r[c:c + 3] = o
    r[d2dhip.SC_PHIMAX] = max(abs(phi_c[0]), abs(phi_c[1]))
    r[d2dhip.SC_VMIN], r[d2dhip.SC_VMAX] = v_c
    r[d2dhip.SC_OKIND], r[d2dhip.SC_BANKMAX] = okind, bankmax
    # x/y_constraint boxes (src/single_opt_planner.py:56-57): soft bound rows like phi / v
    if x_c is not None:
        r[d2dhip.SC_XMIN], r[d2dhip.SC_XMAX] = x_c
    if y_c is not None:
        r[d2dhip.SC_YMIN], r[d2dhip.SC_YMAX] = y_c
    return r


def box_violation(x, y, x_constraint, y_constraint):
    """Largest distance (m) by which the sampled plan leaves the x/y_constraint boxes.  The boxes are soft bound
    rows of the fit (weight W_BOUND, like phi / v), so a binding box is honoured up to a small overshoot that
    the planners report as info['box_violation'] instead of hiding it."""
    v = 0.0
    for val, box in ((x, x_constraint), (y, y_constraint)):
        if box is not None:
            v = max(v, float(box[0] - np.min(val)), float(np.max(val) - box[1]))
    return max(v, 0.0)


def bound_violation(phi, v, phi_constraint, v_constraint):
    """Largest overshoot of the sampled plan beyond phi_constraint (rad) and v_constraint (m/s): like the boxes these are soft
    bound rows of the fit, and a scenario whose bounds bind hard (or conflict) ends in a compromise that the planners report as
    info['phi_violation'] / info['v_violation'] instead of hiding it."""
    vp = max(float(np.max(phi) - phi_constraint[1]), float(phi_constraint[0] - np.min(phi)), 0.0)
    vv = max(float(np.max(v) - v_constraint[1]), float(v_constraint[0] - np.min(v)), 0.0)
    return vp, vv


def dubins_guess(prob):
    """The 'dubins' initial guess of a planner's Problem: node values (n_aircraft, 5, N) and the status per aircraft.  It is a start of
    the collocation problem; the polynomial fit projects its start onto its basis and has no use for one."""
    if not hasattr(prob, 'dubins_guess'):
        raise NotImplementedError("get_initial_guess('dubins') is a start of the collocation backend: build the planner with backend='nlp'")
    return prob.dubins_guess()


class _FitProblem:
    """Stands where the reference keeps its opty Problem (`Planner.prob`): num_free, the two
    option spellings the reference uses, and solve(x0) -> (solution, info)."""

    def __init__(self, planner, n_ac):
        self._p = planner
        self.num_free = 5 * planner.num_nodes * n_ac
        self.options = {'tol': 1e-8, 'max_iter': 200}

    def addOption(self, k, v):
        self.options[k] = v
    add_option = addOption

    def solve(self, x0):
        return self._p._solve(np.asarray(x0, dtype=np.float64))

    # opty's plotting helpers (the reference's `if plot:` branches): out of scope, refused by name
    def _no_plot(self, *_a, **_k):
        raise NotImplementedError('the opty plotting helpers are not part of this backend: plot Planner.sol_* with your own matplotlib code')
    plot_objective_value = plot_trajectories = plot_constraint_violations = _no_plot


class Planner:
    def __init__(self, exp, initialize=True, backend=None, gust=None):
        if gust is not None:
            raise ValueError('a gust is a property of the plant, not of a plan: the planner takes none (fly the plan through it with '
                             'full_sim.implement_controller_batch(gust=...))')
        self.exp = exp
        self.backend = backend or BACKEND
        self.obj_scale = exp.obj_scale
        self.num_nodes, self.time_step, self.duration = d2ou.planner_timing(exp.t0, exp.t1, exp.hz)
        self.wind = exp.wind
        from d2d.wind import planner_wind
        self.field = planner_wind(self.wind)       # None: a constant wind; a class with its own sample_sym that is no spline raises
        if self.field is not None and self.backend == 'fit':
            raise NotImplementedError("backend='fit' cannot plan in a wind field that varies in space and time: the polynomial fit's "
                                      "speed and bank rows would depend on position through the field.  backend='nlp' (or 'auto') "
                                      "solves the collocation problem in the field")
        self.moving_obstacles = check_moving(exp, self.backend)
        self.waypoints = check_waypoints(exp, self.backend)
        # an optional free duration (exp.t1_free = (t1_lo, t1_hi), seconds): the node count stays that of t1 and hz, the time step is
        # an unknown of the collocation problem in [(t1_lo - t0) / (N - 1), (t1_hi - t0) / (N - 1)] (d2d_nlp_solve_free)
        self.t1_free = check_free_time(exp, self.backend)
        # optional hard keep-out discs (exp.keep_out): held by the collocation backend (d2d_nlp_solve_keepout), to which 'auto' goes straight
        self.keep_out = check_keep_out(exp, self.backend, self.moving_obstacles, self.waypoints, self.t1_free)
        # an optional hard geofence (exp.fence): held by the collocation backend (d2d_nlp_solve_fence), to which 'auto' goes straight
        self.fence = check_fence(exp, self.backend, self.moving_obstacles, self.waypoints, self.t1_free, self.keep_out)
        # an optional free duration BESIDE static keep_out discs and a fence (exp.t1_window = (t1_lo, t1_hi), seconds): t1_free's unknown
        # step in the solve that holds both families (d2d_nlp_solve_free_fence); the discs are lowered with the largest step of the window
        self.t1_window = check_window(exp, self.backend, self.moving_obstacles, self.waypoints, self.t1_free, self.field)
        self._free = self.t1_free if self.t1_free is not None else self.t1_window        # the free duration under either spelling
        self.aircraft = d2ou.Aircraft()
        N = self.num_nodes
        self._slice_x, self._slice_y, self._slice_psi, self._slice_phi, self._slice_v = (
            slice(i * N, (i + 1) * N, 1) for i in range(5))
        self.obstacles = exp.obstacles
        # a cost plug-in without a lowering: the collocation problem with the host objective, unless the fit was asked for
        self._host_cost = self.backend != 'fit' and not lowerable(exp.cost)
        if self._host_cost and self.moving_obstacles:
            raise NotImplementedError(MOVING_HOST_COST)
        if self._host_cost and self.waypoints:
            raise NotImplementedError(VIA_HOST_COST)
        if self._host_cost and self.keep_out:
            raise NotImplementedError(KEEP_HOST_COST)
        if self._host_cost and self.fence is not None:
            raise NotImplementedError(FENCE_HOST_COST)
        if initialize and (self.keep_out or self.fence is not None or self.backend == 'nlp' or self._host_cost or self.field is not None or self.moving_obstacles or self.waypoints
                           or self._free is not None):
            import opty.direct_collocation
            _g = self.aircraft
            t0, (x0, y0, psi0, phi0, v0) = exp.t0, exp.p0
            self._instance_constraints = (_g._sx(t0) - x0, _g._sy(t0) - y0, _g._spsi(t0) - psi0)
            t1, (x1, y1, psi1, phi1, v1) = exp.t1, exp.p1
            self._instance_constraints += (_g._sx(t1) - x1, _g._sy(t1) - y1, _g._spsi(t1) - psi1)
            self._instance_constraints += waypoint_constraints(_g, self.waypoints)
            self._bounds = {_g._sphi(_g._st): exp.phi_constraint, _g._sv(_g._st): exp.v_constraint}
            if exp.x_constraint is not None:
                self._bounds[_g._sx(_g._st)] = exp.x_constraint
            if exp.y_constraint is not None:
                self._bounds[_g._sy(_g._st)] = exp.y_constraint
            obj = exp.cost
            step = self.time_step
            if self._free is not None:             # the interval as a symbol with its bound: opty's variable duration
                step = d2ou._Sym('h')
                self._bounds[step] = tuple((t - exp.t0) / (self.num_nodes - 1) for t in self._free)
            self.prob = opty.direct_collocation.Problem(lambda _free: obj.cost(_free, self),
                                                        lambda _free: obj.cost_grad(_free, self),
                                                        _g.get_eom(self.wind), _g._state_symbols, self.num_nodes, step,
                                                        known_parameter_map={}, instance_constraints=self._instance_constraints,
                                                        bounds=self._bounds, parallel=False,
                                                        **(dict(keep_out=self.keep_out) if self.keep_out else {}),
                                                        **(dict(fence=self.fence) if self.fence is not None else {}))
        elif initialize:
            self.prob = _FitProblem(self, 1)

    def _harden(self):
        """backend='auto': the fit's plan overshoots a bound -> the collocation problem (hard bounds), started from that plan."""
        viol = max(self.info.get('box_violation', 0.), self.info.get('phi_violation', 0.), self.info.get('v_violation', 0.))
        self.info['backend_used'] = 'fit'
        if self.backend != 'auto' or not (viol > AUTO_TOL):
            return
        try:
            hard = type(self)(getattr(self, 'exp', None) or self.scen, initialize=True, backend='nlp')
            for k, v in self.prob.options.items():
                if k in ('tol',):
                    hard.prob.addOption(k, v)
            sol, info = hard.prob.solve(self.solution)
        except NotImplementedError as e:     # a cost / bound variant without a collocation kernel: the soft-bound plan stands, and says so
            self.info['nlp_status'] = f'unsupported: {e}'
            return
        st = np.atleast_1d(info['status'])
        info['fit_info'] = self.info
        if (st == 1).all():
            info['backend_used'] = 'nlp'
            self.solution, self.info = sol, info
            # the polynomial of the rejected soft-bound fit no longer describes the plan that is returned (info['fit_info'] keeps
            # its record): fit_q / fit_plan / fit_scen / fit_coefs are valid only when backend_used == 'fit'
            self.fit_q = self.fit_plan = self.fit_scen = self.fit_coefs = None
        else:                              # (e.g. a scenario whose bounds cannot all hold: the soft-bound compromise is what there is)
            self.info['nlp_status'] = info['status']

    def configure(self, tol=1e-8, max_iter=3000):
        self.prob.addOption('tol', tol)
        self.prob.addOption('max_iter', max_iter)

    def get_initial_guess(self, kind='tri'):
        """Node-vector guess [x, y, psi, phi, v] (src/single_opt_planner.py:79-115)."""
        g = np.zeros(self.prob.num_free)
        N = self.num_nodes
        if self._free is not None:                 # the interval is the last entry: the scenario's own step is its start
            g[-1] = self.time_step
        if kind == 'rnd':
            rng = np.random.default_rng(seed)
            cx = self.exp.x_constraint or [-100, 100]
            cy = self.exp.y_constraint or [-100, 100]
            g[self._slice_x] = rng.uniform(cx[0], cx[1], N)
            g[self._slice_y] = rng.uniform(cy[0], cy[1], N)
            g[self._slice_psi] = rng.uniform(-np.pi, np.pi, N)
        elif kind == 'via':
            g[self._slice_x], g[self._slice_y], g[self._slice_psi], g[self._slice_phi], g[self._slice_v] = d2ou.via_guess(
                self.exp.p0, self.exp.p1, self.waypoints, self.exp.t0, self.time_step, N, self.exp.vref)
        elif kind == 'dubins':                     # the row's Dubins path, built on the device (d2d_nlp_guess_dubins)
            W, self.guess_status = dubins_guess(self.prob)
            g[self._slice_x], g[self._slice_y], g[self._slice_psi], g[self._slice_phi], g[self._slice_v] = W[0]
        elif kind == 'tri':
            x, y, psi, phi, v = d2ou.triangle(self.exp.p0[:2], self.exp.p1[:2], self.exp.vref, self.duration, N, go_left=-1.)
            g[self._slice_x], g[self._slice_y], g[self._slice_psi], g[self._slice_phi], g[self._slice_v] = x, y, psi, phi, v
        else:
            g[self._slice_x] = np.linspace(self.exp.p0[0], self.exp.p1[0], N)
            g[self._slice_y] = np.linspace(self.exp.p0[1], self.exp.p1[1], N)
        return g

    def _solve(self, x0):
        low = fit_cost(self.exp.cost)
        ctx = d2dhip.default_context()
        N = self.num_nodes
        s = self.obj_scale / N
        plan = get_plan(N, self.duration, s, low[1], low[2])
        row = scen_row(self.exp.p0, self.exp.p1, self.exp.vref, low, s, self.wind.w, self.exp.phi_constraint,
                       self.exp.v_constraint, x_c=self.exp.x_constraint, y_c=self.exp.y_constraint)
        dsc = ctx.dev(row[None, :])
        xy = np.stack([x0[self._slice_x], x0[self._slice_y]])[None]
        q = plan.project(dsc, ctx.dev(xy))
        max_iter = int(min(max(self.prob.options.get('max_iter', 200), 1), 2000))
        cost, iters, status, stats = plan.solve(dsc, q, max_iter=max_iter)
        _, Xs = plan.sample(dsc, q)
        Xh = Xs.cpu().numpy()[0]
        self.fit_q, self.fit_plan, self.fit_scen = q, plan, dsc
        self.fit_coefs = plan.coeffs(dsc, q).cpu().numpy()[0]
        info = {'status': int(status.cpu().numpy()[0]), 'iters': int(iters.cpu().numpy()[0]),
                'obj_val': float(cost.cpu().numpy()[0]),
                'box_violation': box_violation(Xh[0], Xh[1], self.exp.x_constraint, self.exp.y_constraint),
                'phi_violation': bound_violation(Xh[3], Xh[4], self.exp.phi_constraint, self.exp.v_constraint)[0],
                'v_violation': bound_violation(Xh[3], Xh[4], self.exp.phi_constraint, self.exp.v_constraint)[1], 'status_msg': ('running', 'converged', 'max_iter', 'non-finite', 'stalled')[int(status.cpu().numpy()[0])]}
        return Xs.cpu().numpy()[0].reshape(-1), info

    def run(self, initial_guess=None):
        if initial_guess is None:
            initial_guess = self.get_initial_guess('via' if self.waypoints else 'tri')
        self.solution, self.info = self.prob.solve(initial_guess)
        if self._free is not None:                 # the plan's clock follows the solved interval
            self.time_step = float(self.solution[-1])
            self.duration = self.time_step * (self.num_nodes - 1)
            self.info['backend_used'] = 'nlp'
        elif self._host_cost or self.field is not None or self.moving_obstacles or self.waypoints or self.keep_out or self.fence is not None:
            self.info['backend_used'] = 'nlp'
        elif self.backend != 'nlp':
            self._harden()
        self.interpret_solution()

    def interpret_solution(self):
        self.sol_time = np.linspace(0.0, self.duration, num=self.num_nodes)
        self.sol_x, self.sol_y = self.solution[self._slice_x], self.solution[self._slice_y]
        self.sol_psi, self.sol_phi, self.sol_v = (self.solution[s] for s in (self._slice_psi, self._slice_phi, self._slice_v))

    def save_solution(self, filename):
        wind = np.array([self.wind.sample_num(t, x, y) for t, x, y in zip(self.sol_time, self.sol_x, self.sol_y)])
        extra = {} if self._free is None else dict(time_step=self.time_step, duration=self.duration)
        np.savez(filename, sol_time=self.sol_time, sol_x=self.sol_x, sol_y=self.sol_y, sol_psi=self.sol_psi,
                 sol_phi=self.sol_phi, sol_v=self.sol_v, wind=wind, **extra)
        print('saved {}'.format(filename))

    def load_solution(self, filename):
        d = np.load(filename)
        self.sol_time, self.sol_x, self.sol_y, self.sol_psi, self.sol_phi, self.sol_v = (
            d[k] for k in ('sol_time', 'sol_x', 'sol_y', 'sol_psi', 'sol_phi', 'sol_v'))
        print(f'loaded {filename}')


def compute_or_load(_p, force_recompute=False, filename='/tmp/optyplan.npz', tol=1e-5, max_iter=1500, initial_guess=None):
    """Result cache keyed by file name (src/single_opt_planner.py:152-164)."""
    if force_recompute or not os.path.exists(filename):
        _p.configure(tol, max_iter)
        _p.run(_p.get_initial_guess())
        _p.save_solution(filename)
    else:
        _p.load_solution(filename)


def plot2d(_p, _f=None, _a=None, label=''):
    import matplotlib.pyplot as plt
    _f = _f or plt.figure()
    _a = _a or plt.gca()
    _a.plot(_p.sol_x, _p.sol_y, solid_capstyle='butt', label=label)
    for cx, cy, rm in _p.obstacles:
        _a.add_patch(plt.Circle((cx, cy), rm, color='r', alpha=0.1))
    _a.axis('equal')
    return _f, _a


def plot_chrono(_p, _f=None, _a=None):
    import matplotlib.pyplot as plt
    if _f is None:
        _f, _a = plt.subplots(5, 1)
    for ax, (v, lab) in zip(_a, ((_p.sol_x, 'x'), (_p.sol_y, 'y'), (np.rad2deg(_p.sol_psi), 'psi'),
                                  (np.rad2deg(_p.sol_phi), 'phi'), (_p.sol_v, 'v'))):
        ax.plot(_p.sol_time, v); ax.set_ylabel(lab)
    return _f, _a


exp_0 = d2oscen.exp_0


class exp_1:
    """src/single_opt_planner.py:227-248: the leg of full-sim case 3; p0 is injected by the caller (src/12_full_sim_case3.py:185-190)."""
    name, desc = 'exp 1 - joining 2 points', 'single ac traj computation for test case 2 of full sim'
    ncases = 1
    tol, max_iter = 1e-5, 1500
    vref = 12
    cost, obj_scale = d2ou.CostAirVel(vref), 1
    wind = d2ou.WindField(w=[0, 0])
    obstacles = ()
    t0 = 0
    t1, p1 = 12, (75, 40, 0, 0, 12)
    x_constraint, y_constraint = (-150, 150), (-150, 150)
    v_constraint = (9., 15.)
    phi_constraint = (-np.deg2rad(40.), np.deg2rad(40.))
    initial_guess = 'tri'
    hz = 10

    def set_case(idx): pass
    def label(idx): return ''
