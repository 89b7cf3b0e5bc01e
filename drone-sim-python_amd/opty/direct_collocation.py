"""`opty.direct_collocation.Problem` with the constructor and the members the reference uses (src/single_opt_planner.py:62-71,
76-81,124; src/multi_opt_planner.py:69-78,84-86): the direct-collocation NLP in node variables, solved by d2d_nlp_solve
(csrc/nlp_kernels.hip) instead of sympy code generation + IPOPT.

    Problem(obj, obj_grad, eom, state_symbols, num_nodes, time_step, known_parameter_map=, instance_constraints=, bounds=,
            parallel=False)
    .num_free, .addOption(k, v) / .add_option(k, v), .solve(x0) -> (solution, info)

What is interpreted instead of compiled:
  * eom / state_symbols  -- the fixed kinematic model of d2d.opty_utils.Aircraft.get_eom (an `Eom`: wind, g, aircraft count).  A wind
                            that varies in space and time (eom.field, a d2d.wind.SplineWindField: what its sample_sym put into the
                            equations) is solved by d2d_nlp_solve_wind: one aircraft, lowered objective; node i at t0 + i time_step;
  * instance_constraints -- `x(t) - value` objects: at the smallest and the largest time the end conditions of every aircraft (x, y, psi
                            each); at any time in between a timed waypoint of that aircraft (Problem.waypoints, d2d.opty_utils.Waypoint),
                            which must lie on a node and is held exactly (d2d_nlp_solve_via / d2d_nlp_solve_groups_via);
  * bounds               -- {phi(t): (lo, hi), v(t): ..., x(t): ..., y(t): ..., psi(t): ...}: HARD boxes (primal-dual barrier); the phi
                            interval need not be symmetric (d2d_nlp_opts.bounds carries it and the psi box to the kernel);
  * obj / obj_grad       -- the reference passes closures over a cost plug-in and the planner
                            (`lambda _free: obj.cost(_free, self)`); the plug-in is taken from the closure (or from the explicit
                            `cost=` / `planner=` keywords) and lowered structurally (single_opt_planner.lower_cost): the known
                            classes of d2d.opty_utils / d2d.multiopty_utils have a kernel ("lowered" objective).
                            The gradient the solver follows is the plug-in's cost_grad (reference quirks included, oracle/nlp.py).
                            Any other plug-in, and plain callables with no plug-in behind them, select the HOST objective
                            (`Problem.objective == 'host'`): the host calls obj / obj_grad, as IPOPT does, and the device solves a
                            sequence of quadratic models of them over the exact feasible set (_solve_host, below).
The whole Problem is ONE launch (d2d_nlp_solve_groups): wavefront a of a workgroup solves aircraft a.  The aircraft are coupled
through the objective only -- CostCollision acts on the pair of aircraft 0 and 1, src/d2d/multiopty_utils.py:124-125 -- so the
pair alternates on the device (each turn a full solve against the partner's frozen node positions) until neither moves by more than
options['sweep_tol'] (1e-7 m) or options['max_sweeps'] (12): a fixed point of that alternation is a KKT point of the joint NLP.  A
pair that has not settled is reported 'max_iter'.  A cost that selects its own pairs (CostCollision(pairs=) / CostComposit(col_pairs=))
is lowered to a partner set per aircraft and solved by d2d_nlp_solve_groups_pairs: every aircraft with a partner takes turns against
all of them.  info['min_separation']: per coupled pair, the smallest node-wise distance of the returned plan.
Moving obstacles (the planner's `moving_obstacles`, d2d.opty_utils.MovingObstacle) are lowered to the side table of
d2d_moving_obstacles and solved by d2d_nlp_solve_moving (one aircraft, with or without a field) or d2d_nlp_solve_groups_moving (all
aircraft of the Problem see the same tracks), node i at t0 + i time_step; info['min_clearance']: per disc (per aircraft and disc for
several aircraft) the smallest node-wise distance to the disc's rim.
A VARIABLE DURATION, as upstream opty spells it: `time_step` a symbol (a sympy Symbol, or any object with a `name` that is no number)
instead of a float.  The interval is then the LAST entry of the free vector (num_free = 5 N + 1), may carry a bound in `bounds`
({h_sym: (lo, hi)}; without one: (h / 4, 4 h) of the start value x0[-1]), and is solved with the node values by d2d_nlp_solve_free; a
duration term of the cost (d2d.opty_utils.CostDuration, CostComposit(kdur=)) is its weight.  One aircraft, the constant wind, static
obstacles and a lowered objective: with timed waypoints, moving obstacles, a wind field, the host objective or several aircraft the
constructor raises NotImplementedError naming the combination.  info carries time_step and duration.  keep_out= (static KeepOuts) and
fence= go with it (d2d_nlp_solve_free_fence): the discs are lowered with the LARGEST step of the bound, which the bounds must then
give -- conservative for every step inside it -- and info carries keep_out_clearance / fence_clearance at the solved nodes."""
import numpy as np

import d2dhip

# status codes of include/d2d.h (D2D_ST_*)
ST_CONVERGED, ST_MAXITER, ST_NONFINITE, ST_STALLED = 1, 2, 3, 4
STATUS_MSG = {ST_CONVERGED: 'converged', ST_MAXITER: 'max_iter', ST_NONFINITE: 'non-finite', ST_STALLED: 'stalled'}
# host objective: trust control of the quadratic models (sigma: proximal weight, relative to 1 + the largest curvature entry)
ETA_REJECT, ETA_GOOD = 0.1, 0.75
SIGMA_MIN, SIGMA_MAX, SIGMA_GROW = 1e-3, 1e6, 10.0
STALL_AT_MAX = 2                    # rejections in a row at SIGMA_MAX: STALLED
XTOL, FTOL = 1e-8, 1e-10            # convergence: largest move of an accepted step, change of f relative to 1 + |f|
_HIDX = [(a, c) for a in range(5) for c in range(a, 5)]        # d2d_nlp_model.H planes: upper triangle, row by row


def free_index(n_aircraft, num_nodes, planner=None):
    """int array (n_aircraft, 5, num_nodes): position of (x, y, psi, phi, v)(t_i) of each aircraft in the free vector.  From the
    planner's slices when there is one; otherwise the layout of this package's planners: five planes for one aircraft
    (single_opt_planner), x_a, y_a, psi_a per aircraft then the phi and the v planes for several (multi_opt_planner)."""
    n, N = n_aircraft, num_nodes
    if planner is not None and hasattr(planner, '_slice_x'):
        sl = [planner._slice_x, planner._slice_y, planner._slice_psi, planner._slice_phi, planner._slice_v]
        if not isinstance(sl[0], (list, tuple)):
            sl = [[s] for s in sl]
        return np.stack([np.stack([np.arange(N * n * 5)[sl[c][a]] for c in range(5)]) for a in range(n)])
    if n == 1:
        return np.arange(5 * N).reshape(1, 5, N)
    idx = np.zeros((n, 5, N), dtype=np.int64)
    for a in range(n):
        for c in range(3):
            idx[a, c] = np.arange((c + 3 * a) * N, (c + 3 * a + 1) * N)
        idx[a, 3] = np.arange(3 * n * N + a * N, 3 * n * N + (a + 1) * N)
        idx[a, 4] = np.arange(4 * n * N + a * N, 4 * n * N + (a + 1) * N)
    return idx


def curvature_blocks(grad, x, idx, g0=None):
    """Per-node 5x5 blocks of the Hessian of the function whose gradient is `grad`, by forward differences of grad along coloured
    directions: for each aircraft a, residue r in {0, 1, 2} and component c, component c of every node i = r (mod 3) of aircraft a
    is perturbed at once (step sqrt(eps) max(1, |w|)), and the gradient difference at node i is column c of block i.  Exact up to
    the differencing error when the Hessian couples nodes at most two apart; 15 calls of grad per aircraft.  -> (n, N, 5, 5)
    (not symmetrised).  g0: grad(x) if already known."""
    n, _, N = idx.shape
    g0 = np.asarray(grad(x), dtype=np.float64) if g0 is None else g0
    H = np.zeros((n, N, 5, 5))
    eps = np.sqrt(np.finfo(np.float64).eps)
    for a in range(n):
        for r in range(3):
            nodes = np.arange(r, N, 3)
            for c in range(5):
                pos = idx[a, c, nodes]
                xp = x.copy()
                xp[pos] += eps * np.maximum(1.0, np.abs(x[pos]))
                step = xp[pos] - x[pos]
                dg = np.asarray(grad(xp), dtype=np.float64) - g0
                H[a, nodes, :, c] = (dg[idx[a][:, nodes]] / step).T
    return H


def model_blocks(H, sigma):
    """Symmetrised blocks with their eigenvalues clipped at 0, + sigma I, packed as d2d_nlp_model.H: (n, N, 5, 5) -> (n, 15, N)."""
    S = 0.5 * (H + np.swapaxes(H, -1, -2))
    lam, V = np.linalg.eigh(S)
    S = (V * np.maximum(lam, 0.0)[..., None, :]) @ np.swapaxes(V, -1, -2) + sigma * np.eye(5)
    return np.ascontiguousarray(np.stack([S[..., a, c] for a, c in _HIDX], axis=1))


def _closure_objects(fn):
    out = []
    for c in getattr(fn, '__closure__', None) or ():
        try:
            out.append(c.cell_contents)
        except ValueError:
            pass
    return out


class Problem:
    def __init__(self, obj, obj_grad, eom, state_symbols, num_nodes, time_step, known_parameter_map=None,
                 instance_constraints=(), bounds=None, parallel=False, cost=None, planner=None, keep_out=None, fence=None):
        self.obj, self.obj_grad = obj, obj_grad
        # a symbol for the interval: variable duration (the interval is the last free entry); a number: the fixed step
        self.free_step = time_step if (hasattr(time_step, 'name') and not isinstance(time_step, (int, float, np.number))) else None
        self.num_nodes, self.time_step = int(num_nodes), (float('nan') if self.free_step is not None else float(time_step))
        self.n_aircraft = len(state_symbols) // 3
        self.num_free = 5 * self.num_nodes * self.n_aircraft + (1 if self.free_step is not None else 0)
        self.options = {'tol': 1e-8, 'max_iter': 3000}
        self.wind = tuple(getattr(eom, 'wind', (0., 0.)))
        self.field = getattr(eom, 'field', None)
        if getattr(eom, 'n_aircraft', self.n_aircraft) != self.n_aircraft:
            raise ValueError('eom and state_symbols disagree on the number of aircraft')
        if self.field is not None and self.n_aircraft != 1:
            raise NotImplementedError('a wind field that varies in space and time is planned for one aircraft at a time '
                                      '(d2d_nlp_solve_wind): the multi-aircraft Problem and its CostCollision partner '
                                      '(d2d_nlp_solve_groups) take a constant wind')
        # the cost plug-in and the planner behind the obj closure (the reference's call sites close over both)
        if cost is None or planner is None:
            for o in _closure_objects(obj):
                if cost is None and hasattr(o, 'cost') and hasattr(o, 'cost_grad'):
                    cost = o
                if planner is None and hasattr(o, 'num_nodes') and hasattr(o, 'obj_scale'):
                    planner = o
        self.cost, self.planner = cost, planner
        self.moving = list(getattr(planner, 'moving_obstacles', None) or [])
        # a known plug-in behind a planner: its kernel ('lowered'); anything else: the host calls obj / obj_grad ('host')
        self.objective = 'host'
        if cost is not None and planner is not None:
            import single_opt_planner as sop
            try:
                sop.lower_cost(cost)
                self.objective = 'lowered'
            except NotImplementedError:
                pass
        # end conditions per aircraft from the instance constraints: names x<i>, y<i>, psi<i>
        ids = [str(s.sym.name)[1:] for s in state_symbols[0::3]]
        t_all = sorted({c.t for c in instance_constraints})
        if len(t_all) < 2:
            raise NotImplementedError('instance constraints at two times at least (t0 and t1: the end conditions) are required')
        self.t_start = float(t_all[0])                  # node i is at t_start + i time_step (what a field is sampled at)
        self.p0s = np.zeros((self.n_aircraft, 3)); self.p1s = np.zeros((self.n_aircraft, 3))
        seen = set()
        pins = [{} for _ in range(self.n_aircraft)]     # per aircraft: time -> {component name: value}
        for c in instance_constraints:
            for k, nm in enumerate(('x', 'y', 'psi')):
                for a, i in enumerate(ids):
                    if c.name == nm + i:
                        if c.t in (t_all[0], t_all[-1]):
                            (self.p0s if c.t == t_all[0] else self.p1s)[a, k] = c.value
                            seen.add((a, k, c.t == t_all[0]))
                        elif nm in pins[a].setdefault(float(c.t), {}):
                            raise ValueError(f'{c.name} is fixed twice at t = {c.t}')
                        else:
                            pins[a][float(c.t)][nm] = float(c.value)
        if len(seen) != 6 * self.n_aircraft:
            raise NotImplementedError('every aircraft needs x, y, psi fixed at t0 and t1 (src/single_opt_planner.py:46-49)')
        # every other time: pins of that aircraft, which must lie on interior nodes (ValueError otherwise)
        import d2d.opty_utils as d2ou
        self.waypoints = [[d2ou.Waypoint(t, **pa[t]) for t in sorted(pa)] for pa in pins]
        self.via = None                                 # (n_aircraft, n_via, 5): the table of d2d_via_points
        if any(self.waypoints) and self.free_step is not None:
            raise NotImplementedError(f'a variable duration (time_step = {self.free_step}) together with instance_constraints at interior '
                                      'times (a timed waypoint changes node with the step) is not supported')
        if any(self.waypoints):
            n_via = max(len(w) for w in self.waypoints)
            self.via = np.stack([d2ou.lower_waypoints(w, self.t_start, self.time_step, self.num_nodes, n_via) for w in self.waypoints])
        # bounds per aircraft
        self.bounds = [{} for _ in range(self.n_aircraft)]
        self.step_bounds = None                        # (lo, hi) of a free interval, or None: (h / 4, 4 h) of the start value
        for key, (lo, hi) in (bounds or {}).items():
            if self.free_step is not None and (key is self.free_step or (not hasattr(key, 'sym') and key == self.free_step)):
                self.step_bounds = (float(lo), float(hi))
                if not 0.0 < self.step_bounds[0] < self.step_bounds[1]:
                    raise ValueError(f'bounds of the time step {key}: 0 < lo < hi required, got {self.step_bounds}')
                continue
            for nm in ('phi', 'psi', 'v', 'x', 'y'):
                for a, i in enumerate(ids):
                    if key.sym.name == nm + i:
                        self.bounds[a][nm] = (float(lo), float(hi))
        for bd in self.bounds:
            if 'phi' not in bd or 'v' not in bd:
                raise NotImplementedError('phi and v bounds are required (the model divides by v)')
        # hard keep-out discs (d2d.opty_utils.KeepOut): true inequalities of the NLP, held at the nodes (d2d_nlp_solve_keepout)
        self.keep_out = list(keep_out or [])
        if self.keep_out:
            what = ('more than one aircraft' if self.n_aircraft != 1 else
                    'moving obstacles' if self.moving else
                    'instance_constraints at interior times (waypoints)' if self.via is not None else
                    'the host objective (a cost plug-in without a kernel)' if self.objective == 'host' else None)
            if what:
                raise NotImplementedError(f'keep_out together with {what} is not supported')
            import d2d.opty_utils as d2ou
            # a list with a MovingKeepOut plans through d2d_nlp_solve_keepout_moving: every disc as a track (a static one stands still)
            self.keep_moving = any(isinstance(k, d2ou.MovingKeepOut) for k in self.keep_out)
            if self.free_step is not None:
                # a variable duration holds STATIC hard discs (d2d_nlp_solve_free_fence).  The chord between two nodes grows with the
                # step: the discs are lowered with the LARGEST step of its bound, which is conservative for every step inside it
                if self.keep_moving:
                    raise NotImplementedError(f'a MovingKeepOut in keep_out together with a variable duration (time_step = {self.free_step}) '
                                              'is not supported: its centre at a node depends on the step')
                if self.step_bounds is None:
                    raise ValueError(f'keep_out together with a variable duration needs bounds={{{self.free_step}: (lo, hi)}}: the discs are '
                                     'lowered for the largest step')
                self.keep_rows = d2ou.lower_keep_out(self.keep_out, self.bounds[0]['v'][1], self.step_bounds[1])
            elif self.keep_moving:
                self.keep_knots, self.keep_disc = d2ou.lower_keep_moving(self.keep_out, self.bounds[0]['v'][1], self.time_step)
            else:
                self.keep_rows = d2ou.lower_keep_out(self.keep_out, self.bounds[0]['v'][1], self.time_step)
        # a hard geofence (d2d.opty_utils.GeoFence, or its lowered rows): every node inside the convex polygon (d2d_nlp_solve_fence; with
        # several aircraft d2d_nlp_solve_groups_fence: one polygon for all of them)
        self.fence = fence
        if fence is not None:
            what = ('moving obstacles' if self.moving else
                    'instance_constraints at interior times (waypoints)' if self.via is not None else
                    'the host objective (a cost plug-in without a kernel)' if self.objective == 'host' else
                    'a MovingKeepOut in keep_out (hard discs that move)' if self.keep_out and self.keep_moving else None)
            if what:
                raise NotImplementedError(f'fence together with {what} is not supported')
            import d2d.opty_utils as d2ou
            self.fence_rows = d2ou.lower_fence(fence)
        if self.free_step is not None:                  # what a free interval is not combined with (d2d_nlp_solve_free, _free_fence)
            what = ('more than one aircraft (they share one interval: the joint system is not built)' if self.n_aircraft != 1 else
                    'moving obstacles (their node times move with the step)' if self.moving else
                    'a wind field that varies in space and time (its time derivative enters the border)' if self.field is not None else
                    'the host objective (a cost plug-in without a kernel)' if self.objective == 'host' else None)
            if what:
                raise NotImplementedError(f'a variable duration (time_step = {self.free_step}) together with {what} is not supported')

    def addOption(self, k, v):
        self.options[k] = v
    add_option = addOption

    # opty's plotting helpers (called by the reference's `if plot:` branches, src/06_optyplan.py:159-161, src/07_multioptyplan.py:
    # 90-92): plotting is out of scope -- refuse by name instead of failing with an AttributeError
    def _no_plot(self, *_a, **_k):
        raise NotImplementedError('opty.direct_collocation.Problem plotting helpers are not part of this backend: plot Planner.sol_* '
                                  '(x, y, psi, phi, v over sol_time) with your own matplotlib code')
    plot_objective_value = plot_trajectories = plot_constraint_violations = _no_plot

    def _rows(self):
        import single_opt_planner as sop
        low = sop.lower_cost(self.cost)
        n, N = self.n_aircraft, self.num_nodes
        multi = hasattr(self.planner, 'acs')
        s = self.planner.obj_scale / N / (n if multi else 1)
        rows = []
        for a in range(n):
            la = low if (a == 0 or not multi) else low[:4] + ((),) + low[5:]     # static obstacles act on aircraft 0 only (multi, :74)
            bd = self.bounds[a]
            r = sop.scen_row(tuple(self.p0s[a]) + (0., 0.), tuple(self.p1s[a]) + (0., 0.), 0., la, s, self.wind, bd['phi'], bd['v'],
                             x_c=bd.get('x'), y_c=bd.get('y'))
            if multi and la[4]:
                r[d2dhip.SC_KOBS] *= n                                             # obstacle scale has no 1/n_ac (:91)
            rows.append(r)
        rows = np.stack(rows)
        coupled = multi and n >= 2 and not np.isnan(low[5]) and low[5] > 0
        self._pairs = sop.collision_pairs_of(low, n) if coupled else None      # None: the reference's pair (0, 1)
        if coupled and self._pairs is None:
            rows[:2, d2dhip.SC_KCOL], rows[:2, d2dhip.SC_RCOL], rows[:2, d2dhip.SC_SCOL] = low[5], low[6], self.planner.obj_scale / N
        elif coupled:
            # CostCollision(pairs=): every aircraft with a partner carries the collision columns and its symmetric partner set
            # (d2d_nlp_solve_groups_pairs)
            if n > 8:
                raise NotImplementedError('collision coupling is built for groups of at most 8 aircraft')
            import d2d.multiopty_utils as d2mou
            for a, m in enumerate(d2mou.pair_masks(self._pairs, n)):
                if m:
                    rows[a, d2dhip.SC_KCOL], rows[a, d2dhip.SC_RCOL], rows[a, d2dhip.SC_SCOL] = low[5], low[6], self.planner.obj_scale / N
                    rows[a, d2dhip.SC_PMASK] = m
            coupled = len(self._pairs) > 0
        # (low[8]: CostBank(use_mean=False) travels as D2D_SC_BANKMAX -- obj_scale kbank max phi^2 with the maximiser frozen for the
        # length of a Newton step, csrc/nlp_kernels.hip nlp_assemble / oracle/nlp.py)
        return rows, coupled

    def dubins_guess(self):
        """Node values (n_aircraft, 5, N) of the Dubins start of every aircraft and its status per aircraft (d2d_nlp_guess_dubins on the
        rows and the bounds table of solve(); a free interval at the planner's own step).  What a Dubins path does not know is refused
        by name."""
        what = ('a wind field that varies in space and time (the guess is built in the air frame of a constant wind)' if self.field is not None else
                'moving obstacles' if self.moving else
                "waypoints (the 'via' guess is the one that knows pins)" if self.via is not None else
                'hard keep-out discs (the path would have to go round them)' if self.keep_out else
                'a geofence (the path would have to stay inside it)' if self.fence is not None else None)
        if what:
            raise NotImplementedError(f"the 'dubins' initial guess together with {what} is not supported")
        rows, bnd = (self._rows()[0], self._bounds_table()) if self.objective == 'lowered' else self._host_rows()
        ctx = d2dhip.default_context()
        W, out = ctx.nlp_guess_dubins(ctx.dev(rows), self.num_nodes, float(self.planner.time_step), bounds=None if bnd is None else ctx.dev(bnd),
                                      outputs=('status',))
        ctx.sync()
        status = out['status'].cpu().numpy()
        if (status == d2dhip.GUESS_INVALID).any():
            raise ValueError(f"the 'dubins' initial guess refuses the rows of aircraft {np.flatnonzero(status == d2dhip.GUESS_INVALID).tolist()} "
                             '(non-finite entries, v bounds or a phi interval without a bank to either side)')
        return W.cpu().numpy(), status

    def _solver_kw(self):
        """The solver options of every path, from IPOPT's.  Its max_iter counts Newton steps; here they are grouped as outer (multiplier /
        barrier updates) x inner (<= D2D_NLP_INNER_MAX): between 720 and 3600 steps in all, as in rounds 2-3 (12 .. 60 batches of 60).
        Its `tol` (the reference sets 1e-5 .. 1e-8) bounds its scaled KKT error.  This backend's own tolerances -- barrier KKT error of the
        last inner problem 1e-7, collocation residual 1e-9 -- are at least as tight as every value the reference uses, so a looser `tol`
        changes nothing; a tighter one tightens them with it."""
        _im = d2dhip.NLP_INNER_MAX
        tol = float(self.options.get('tol', 1e-8))
        return dict(inner_max=_im, outer_max=int(min(max(self.options.get('max_iter', 3000) // _im, 720 // _im), 3600 // _im)),
                    opt_tol=min(tol, 1e-7), feas_tol=min(1e-2 * tol, 1e-9))

    def _bounds_table(self):
        """(n_aircraft, 4) = (phi_lo, phi_hi, psi_lo, psi_hi): an asymmetric phi interval / a box on psi travel beside the rows
        (d2d_nlp_opts.bounds; lo >= hi: not set).  None when no aircraft has either."""
        if not any('psi' in bd or abs(bd['phi'][0] + bd['phi'][1]) > 1e-12 for bd in self.bounds):
            return None
        return np.array([[bd['phi'][0], bd['phi'][1]] + list(bd.get('psi', (0.0, 0.0))) for bd in self.bounds], dtype=np.float64)

    def solve(self, x0):
        if self.objective == 'host':
            if self.moving:
                import single_opt_planner as sop
                raise NotImplementedError(sop.MOVING_HOST_COST)
            if self.via is not None:
                import single_opt_planner as sop
                raise NotImplementedError(sop.VIA_HOST_COST)
            if self.field is not None:
                raise NotImplementedError('a wind field that varies in space and time together with a host objective (a cost plug-in '
                                          'without a kernel, d2d_nlp_solve_model) is not supported: use one of the cost classes of '
                                          'd2d.opty_utils, or a constant wind')
            return self._solve_host(np.asarray(x0, dtype=np.float64))
        ctx = d2dhip.default_context()
        n, N = self.n_aircraft, self.num_nodes
        x0 = np.asarray(x0, dtype=np.float64)
        sl = self.planner
        single = not isinstance(sl._slice_x, (list, tuple))
        get = (lambda s, a: x0[s]) if single else (lambda s, a: x0[s[a]])
        W = np.stack([np.stack([get(sl._slice_x, a), get(sl._slice_y, a), get(sl._slice_psi, a), get(sl._slice_phi, a),
                                get(sl._slice_v, a)], 0) for a in range(n)], 0)                       # (n, 5, N)
        rows, coupled = self._rows()
        if self.free_step is not None:
            return self._solve_free(ctx, x0, W, rows)
        kw = self._solver_kw()
        bnd = self._bounds_table()
        kw['bounds'] = None if bnd is None else ctx.dev(bnd)
        dsc = ctx.dev(rows)
        dW = ctx.dev(np.ascontiguousarray(W))
        if not coupled:
            dsc[:, d2dhip.SC_KCOL] = 0.0
        multi = hasattr(self.planner, 'acs')
        tabled = bool(self.moving) or self.via is not None   # tracks and pins travel beside the rows; node i at t_start + i time_step
        # A lone aircraft with pins, discs or a field takes the hand-out entries (in a field the rows' NaN wind columns are not read).
        # Everything else is ONE launch of a group entry: wavefront a of a workgroup solves aircraft a; the aircraft coupled by
        # CostCollision alternate on the device (block Gauss-Seidel) until none moves -- the pair (0, 1), or with a cost that selects
        # its own pairs every aircraft with a partner.
        group = False if self.keep_out else n > 1 if self.fence is not None else multi if tabled else self.field is None
        ex = dict(field=self.field, t_start=self.t_start if (self.moving or self.field is not None) else None)
        if self.keep_out and self.keep_moving:
            ex.update(hard_knots=ctx.dev(self.keep_knots[None]), hard_disc=ctx.dev(self.keep_disc[None]), t_start=self.t_start)
        elif self.keep_out:
            ex['keep'] = ctx.dev(self.keep_rows[None])
        if self.fence is not None:                # one polygon for the problem: every aircraft of the scenario holds it
            ex['fence'] = ctx.dev(self.fence_rows[None])
        if self.moving:
            import d2d.opty_utils as d2ou
            knots, disc = d2ou.lower_moving(self.moving)
            ex.update(knots=ctx.dev(knots[None]), disc=ctx.dev(disc[None]))
        if self.via is not None:
            ex['via'] = ctx.dev(self.via)
        if group:
            if (tabled or self.fence is not None) and coupled and self._pairs is None:       # (these entries read the partner sets: the pair (0, 1) as such)
                import d2d.multiopty_utils as d2mou
                d2mou.default_pair_masks(dsc, n, True)
            ex.update(n_ac=n, pairs=self._pairs is not None, max_sweeps=int(self.options.get('max_sweeps', 12)),
                      tol=float(self.options.get('sweep_tol', 1e-7)))
        out = d2dhip.nlp_plan(ctx, dsc, dW, self.time_step, **ex, **kw)
        sweeps, moved = (int(out['sweeps'][0].item()), float(out['moved'][0].item())) if group else (0, 0.0)
        ctx.sync()
        Wh = dW.cpu().numpy()
        sol = np.zeros(self.num_free)
        for a in range(n):
            for c, s in enumerate((sl._slice_x, sl._slice_y, sl._slice_psi, sl._slice_phi, sl._slice_v)):
                sol[s if single else s[a]] = Wh[a, c]
        st = out['status'].cpu().numpy()
        info = {'status': int(st.max()) if single else st.tolist(), 'feas': float(out['feas'].max().item()),
                'iters': out['iters'].cpu().numpy().tolist(), 'sweeps': sweeps, 'moved': moved,
                'obj_val': float(self.obj(sol)), 'status_msg': 'converged' if (st == 1).all() else 'max_iter',
                'box_violation': 0.0, 'phi_violation': 0.0, 'v_violation': 0.0}       # hard bounds: an interior-point iterate never leaves its box
        if coupled:                               # per coupled pair: the smallest node-wise distance of the returned plan
            info['min_separation'] = {(i, j): float(np.hypot(Wh[i, 0] - Wh[j, 0], Wh[i, 1] - Wh[j, 1]).min())
                                      for i, j in (self._pairs if self._pairs is not None else [(0, 1)])}
        if self.moving:                           # the device's cost carries the discs' terms; the plug-in's value does not
            import d2d.opty_utils as d2ou
            tn = self.t_start + np.arange(N) * self.time_step
            mc = [d2ou.min_clearance(self.moving, tn, Wh[a, 0], Wh[a, 1]) for a in range(n)]
            info['min_clearance'] = mc if multi else mc[0]
            info['cost'] = float(out['cost'].sum().item())
        if self.keep_out:                         # per disc: the polyline's clearance from the user's disc (>= its margin)
            import d2d.opty_utils as d2ou
            if self.keep_moving:                  # continuous in time, against the moving centre
                info['keep_out_clearance'] = d2ou.moving_keep_clearance(self.keep_out, self.t_start + np.arange(N) * self.time_step, Wh[0, 0], Wh[0, 1])
            else:
                info['keep_out_clearance'] = d2ou.keep_out_clearance(self.keep_out, Wh[0, 0], Wh[0, 1])
        if self.fence is not None:                # per edge: the nodes' distance from the user's polygon (>= its margin; by convexity the polyline's too)
            import d2d.opty_utils as d2ou
            fc = [d2ou.fence_clearance(self.fence, Wh[a, 0], Wh[a, 1]) for a in range(n)]
            info['fence_clearance'] = fc if multi else fc[0]
        if self.via is not None:                  # 0.0 by construction: a pinned component never leaves its value
            import d2d.opty_utils as d2ou
            info['waypoint_error'] = max(d2ou.waypoint_error(self.via[a], Wh[a]) for a in range(n))
        return sol, info

    def _solve_free(self, ctx, x0, W, rows):
        """The variable-duration Problem: one aircraft, the interval x0[-1] free in its bound (d2d_nlp_solve_free; with static hard discs
        or a geofence d2d_nlp_solve_free_fence, through nlp_plan's window=)."""
        import single_opt_planner as sop
        N = self.num_nodes
        h0 = float(x0[-1])
        if not (np.isfinite(h0) and h0 > 0.0):
            raise ValueError(f'the start value of the time step (the last entry of x0) must be positive and finite, got {h0}')
        lo, hi = self.step_bounds if self.step_bounds is not None else (h0 / 4.0, 4.0 * h0)
        bnd = self._bounds_table()
        dsc = ctx.dev(rows)
        dsc[:, d2dhip.SC_KCOL] = 0.0
        dW = ctx.dev(np.ascontiguousarray(W))
        self.free_rows = np.array([[lo, hi, sop.duration_weight(sop.lower_cost(self.cost)), h0]])
        if self.keep_out or self.fence is not None:
            out = d2dhip.nlp_plan(ctx, dsc, dW, h0, window=ctx.dev(self.free_rows), keep=ctx.dev(self.keep_rows[None]) if self.keep_out else None,
                                  fence=None if self.fence is None else ctx.dev(self.fence_rows[None]), bounds=None if bnd is None else ctx.dev(bnd),
                                  **self._solver_kw())
        else:
            out = d2dhip.nlp_plan(ctx, dsc, dW, h0, free_rows=ctx.dev(self.free_rows), bounds=None if bnd is None else ctx.dev(bnd), **self._solver_kw())
        ctx.sync()
        Wh = dW.cpu().numpy()
        h = float(out['h'][0].item())
        sl = self.planner
        sol = np.zeros(self.num_free)
        for c, s in enumerate((sl._slice_x, sl._slice_y, sl._slice_psi, sl._slice_phi, sl._slice_v)):
            sol[s] = Wh[0, c]
        sol[-1] = h
        st = int(out['status'][0].item())
        info = {'status': st, 'feas': float(out['feas'][0].item()), 'iters': out['iters'].cpu().numpy().tolist(), 'sweeps': 0,
                'moved': 0.0, 'obj_val': float(self.obj(sol)), 'cost': float(out['cost'][0].item()),
                'status_msg': STATUS_MSG.get(st, 'max_iter'), 'time_step': h, 'duration': h * (N - 1),
                'box_violation': 0.0, 'phi_violation': 0.0, 'v_violation': 0.0}
        if self.keep_out or self.fence is not None:       # the clearances of the fixed-step solve, at the solved nodes
            import d2d.opty_utils as d2ou
            if self.keep_out:
                info['keep_out_clearance'] = d2ou.keep_out_clearance(self.keep_out, Wh[0, 0], Wh[0, 1])
            if self.fence is not None:
                info['fence_clearance'] = d2ou.fence_clearance(self.fence, Wh[0, 0], Wh[0, 1])
        return sol, info

    # ---- host objective ------------------------------------------------------------------------------------------------------
    def _host_rows(self):
        """Scenario rows with every structured cost weight 0 (the objective is the model alone) + the bounds beside them."""
        import single_opt_planner as sop
        low = (0., 0., 0., 0., (), float('nan'), 0., 0, 0)
        rows = np.stack([sop.scen_row(tuple(self.p0s[a]) + (0., 0.), tuple(self.p1s[a]) + (0., 0.), 0., low, 1.0, self.wind,
                                      bd['phi'], bd['v'], x_c=bd.get('x'), y_c=bd.get('y')) for a, bd in enumerate(self.bounds)])
        return rows, self._bounds_table()

    def _solve_host(self, x0):
        """A sequence of quadratic models of the user's objective over the exact feasible set (the collocation equalities, end
        conditions and hard boxes), each solved on the device by d2d_nlp_solve_model -- one launch for all aircraft:
          0. restoration: the start projected onto the feasible set (g = 0, H = I), so that every iterate W_k is feasible;
          1. at W_k: f_k = obj, g_k = obj_grad (one call each), per-node curvature blocks from 15 obj_grad calls per aircraft
             (curvature_blocks), symmetrised, eigenvalues clipped at 0, + sigma I;
          2. W_new = argmin g_k.d + 1/2 d^T H d over the feasible set, from W_k;
          3. ratio test with the true obj (both points feasible): rho = (f_k - f(W_new)) / (m(W_k) - m(W_new)); rho < 0.1: rejected,
             sigma grows and the model is solved again; rho > 0.75: sigma shrinks.
        Stops: converged (an accepted step that changes f by <= FTOL (1 + |f|) and moves no variable by more than XTOL, or of which
        the model itself predicted no more than that), max_iter (outer cap from options['max_iter']), stalled (the subproblem
        found no feasible point, or STALL_AT_MAX rejections in a row at the largest sigma: e.g. an obj_grad that is not the gradient
        of obj), non-finite (obj or obj_grad not finite at an iterate; a non-finite obj at a trial point is a rejection)."""
        ctx = d2dhip.default_context()
        n, N = self.n_aircraft, self.num_nodes
        idx = free_index(n, N, self.planner)
        rows, bnd = self._host_rows()
        dsc = ctx.dev(rows)
        dbnd = None if bnd is None else ctx.dev(bnd)
        kw = dict(self._solver_kw(), bounds=dbnd)
        outer_cap = int(self.options.get('outer_max', min(max(int(self.options.get('max_iter', 3000)) // 20, 8), 100)))
        calls = {'cost': 0, 'grad': 0}

        def f_of(x):
            calls['cost'] += 1
            return float(np.asarray(self.obj(x), dtype=np.float64))

        def g_of(x):
            calls['grad'] += 1
            return np.asarray(self.obj_grad(x), dtype=np.float64).reshape(-1)

        def to_free(W):
            x = x0.copy()
            x[idx] = W
            return x

        iters = np.zeros(n, dtype=np.int64)
        sub_iters = []
        feas = np.zeros(n)

        def sub(Wc, g, Hp):
            dW = ctx.dev(np.ascontiguousarray(Wc))
            out = ctx.nlp_solve_model(dsc, dW, self.time_step, ctx.dev(np.ascontiguousarray(g)), ctx.dev(Hp), ctx.dev(np.ascontiguousarray(Wc)), **kw)
            ctx.sync()
            it = out['iters'].cpu().numpy()
            iters[:] += it
            sub_iters.append(int(it.max()))
            feas[:] = out['feas'].cpu().numpy()
            return dW.cpu().numpy(), float(out['cost'].sum().item()), out['status'].cpu().numpy()

        # 0. restoration of the start
        W0 = x0[idx]
        eye = np.zeros((n, 15, N))
        for k, (a, c) in enumerate(_HIDX):
            if a == c:
                eye[:, k] = 1.0
        Wk, _, st = sub(W0, np.zeros_like(W0), eye)
        status, outer, f, sigma = ST_MAXITER, 0, float('nan'), 0.0
        if (st == ST_NONFINITE).any() or not np.isfinite(Wk).all():
            status = ST_NONFINITE
        elif (st == ST_STALLED).any():
            status = ST_STALLED
        else:
            xk = to_free(Wk)
            f, g = f_of(xk), g_of(xk)
            status = None
            if not (np.isfinite(f) and np.isfinite(g).all()):
                status = ST_NONFINITE
            else:
                Hraw = curvature_blocks(g_of, xk, idx, g0=g)
            n_max = 0
            while status is None:
                if not np.isfinite(Hraw).all():
                    status = ST_NONFINITE
                    break
                if outer >= outer_cap:
                    status = ST_MAXITER
                    break
                outer += 1
                hs = 1.0 + float(np.abs(Hraw).max())
                Wn, m_new, st = sub(Wk, g[idx], model_blocks(Hraw, sigma * hs))
                if (st == ST_STALLED).any():
                    status = ST_STALLED
                    break
                ftol = FTOL * (1.0 + abs(f))
                pred = -m_new
                ok = not (st == ST_NONFINITE).any() and (st == ST_CONVERGED).all() and np.isfinite(Wn).all()
                f_new = f_of(to_free(Wn)) if ok else float('nan')
                ared = f - f_new
                if not np.isfinite(f_new):
                    accept, ratio = False, -np.inf
                elif pred <= ftol:                  # the model sees nothing left to gain: a step that does not raise f is taken
                    accept, ratio = ared >= -ftol, 1.0
                else:
                    ratio = ared / pred
                    accept = ratio >= ETA_REJECT
                if not accept:
                    if sigma >= SIGMA_MAX:
                        n_max += 1
                        if n_max >= STALL_AT_MAX:
                            status = ST_STALLED
                            break
                    sigma = min(max(sigma * SIGMA_GROW, SIGMA_MIN), SIGMA_MAX)
                    continue
                n_max = 0
                move = float(np.abs(Wn - Wk).max())
                Wk, xk = Wn, to_free(Wn)
                if abs(ared) <= ftol and (move <= XTOL or pred <= ftol):
                    f = f_new
                    status = ST_CONVERGED
                    break
                f, g = f_new, g_of(xk)
                if not np.isfinite(g).all():
                    status = ST_NONFINITE
                    break
                Hraw = curvature_blocks(g_of, xk, idx, g0=g)
                if ratio > ETA_GOOD:
                    sigma = sigma / SIGMA_GROW if sigma > SIGMA_MIN else 0.0
        sol = to_free(Wk)
        info = {'status': int(status) if n == 1 else [int(status)] * n, 'feas': float(feas.max()), 'iters': iters.tolist(),
                'sweeps': 0, 'moved': 0.0, 'obj_val': f, 'status_msg': STATUS_MSG[status],
                'box_violation': 0.0, 'phi_violation': 0.0, 'v_violation': 0.0,
                'objective': 'host', 'outer': outer, 'cost_calls': calls['cost'], 'grad_calls': calls['grad'], 'sub_iters': sub_iters}
        return sol, info
