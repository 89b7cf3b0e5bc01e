"""Mirror of src/d2d/opty_utils.py (reference): planner timing, wind, the aircraft symbol
holder, the single-aircraft cost plug-ins and the 'triangle' initial guess.

The cost classes keep the reference's plug-in protocol -- cost(free, planner) and
cost_grad(free, planner) on the node vector [x, y, psi, phi, v] -- so that user code and the
reference's own fake-planner checks (src/test/test_objective.py) keep working.  The planners
recognise these classes structurally and lower them to kernel parameters
(single_opt_planner.lower_cost); their gradients reproduce the reference's expressions,
including where those differ from the true derivative."""
import numpy as np


def planner_timing(t0, t1, hz):
    """Node count, step and rounded duration (src/d2d/opty_utils.py:8-14)."""
    num_nodes = int((t1 - t0) * hz) + 1
    time_step = 1. / hz
    duration = (num_nodes - 1) * time_step
    print(f'time_step: {time_step:.3f}s ({hz:.1f}hz), duration {duration:.1f}s -> {num_nodes} nodes')
    return num_nodes, time_step, duration


class WindField:
    def __init__(self, w=[0., 0.]):
        self.w = w

    def sample_sym(self, _t, _x, _y):
        return self.w

    def sample_num(self, _t, _x, _y):
        return self.w

    def __str__(self):
        return f'{self.w} m/s'


class _Sym:
    """Named placeholder standing where the reference holds a sympy Function / Symbol.  No computer algebra is needed on this
    side -- the model is fixed (the three kinematic equations below) and lives in the kernels -- but the reference's planner
    code builds its instance constraints and bounds out of these objects (`_g._sx(t0) - x0`, `bounds[_g._sphi(_g._st)] = ...`,
    src/single_opt_planner.py:46-57), so they support exactly that: calling (-> the function at a time), subtraction of a
    number (-> an instance constraint), hashing (-> keys of the bounds dictionary)."""

    def __init__(self, name):
        self.name = name

    def __call__(self, t=None):
        return _SymAt(self, t)

    def __repr__(self):
        return self.name


class _SymAt:
    """`x(t)`: a state / input function at a time (a number for instance constraints, the time symbol for bounds)."""

    def __init__(self, sym, t):
        self.sym, self.t = sym, t

    def __sub__(self, value):
        return InstanceConstraint(self.sym.name, self.t, float(value))

    def __hash__(self):
        return hash((self.sym.name, repr(self.t)))

    def __eq__(self, other):
        return isinstance(other, _SymAt) and (self.sym.name, repr(self.t)) == (other.sym.name, repr(other.t))

    def diff(self):
        return _SymAt(_Sym(self.sym.name + "'"), self.t)

    def __repr__(self):
        return f'{self.sym.name}({self.t})'


class InstanceConstraint:
    """`name(t) - value = 0` (what `_g._sx(t0) - x0` evaluates to)."""

    def __init__(self, name, t, value):
        self.name, self.t, self.value = name, float(t), value

    def __repr__(self):
        return f'{self.name}({self.t}) - {self.value}'


class Eom(tuple):
    """The symbolic model of the reference (src/d2d/opty_utils.py:38-50) as data: residual form, wind entering with a + sign
    (the reference's quirk: the plant, src/d2d/dynamic.py:18-19, has the opposite sign).  A tuple of printable equations that
    also carries what the solver needs: the wind vector and g.  A wind that varies in space and time (what
    d2d.wind.SplineWindField.sample_sym returns) is kept as eom.field; eom.wind is NaN then: no constant stands for a field."""

    def __new__(cls, wind, g=9.81, ids=('',)):
        eqs = []
        for i in ids:
            eqs += [f"x{i}' - v{i} cos(psi{i}) + {wind[0]}", f"y{i}' - v{i} sin(psi{i}) + {wind[1]}", f"psi{i}' - {g}/v{i} tan(phi{i})"]
        self = super().__new__(cls, eqs)
        self.field = getattr(wind, 'field', None)
        self.wind = (float(wind[0]), float(wind[1])) if self.field is None else (float('nan'), float('nan'))
        self.g, self.n_aircraft = g, len(ids)
        return self


class Aircraft:
    """Symbol holder of one aircraft (src/d2d/opty_utils.py:31-50): states (x, y, psi), inputs (v, phi)."""

    def __init__(self, st=None, id=''):
        self._st = st or _Sym('t')
        self._id = id
        self._sx, self._sy, self._sv, self._sphi, self._spsi = (_Sym(f'{n}{id}') for n in ('x', 'y', 'v', 'phi', 'psi'))
        self._state_symbols = (self._sx(self._st), self._sy(self._st), self._spsi(self._st))
        self._input_symbols = (self._sv, self._sphi)

    def get_eom(self, atm, g=9.81):
        """xdot - v cos(psi) + wx, ydot - v sin(psi) + wy, psidot - g/v tan(phi)  (residual form, :42-44)."""
        return Eom(atm.sample_sym(self._st, self._sx(self._st), self._sy(self._st)), g, (self._id,))


# ---------------------------------------------------------------------------------------
# cost plug-ins.  s = obj_scale / num_nodes throughout.
# ---------------------------------------------------------------------------------------
class CostAirVel:
    """s * sum (v - vsp)^2  (src/d2d/opty_utils.py:55-66)."""

    def __init__(self, vsp=10.):
        self.vsp = vsp

    def cost(self, free, _p):
        return _p.obj_scale * np.sum((free[_p._slice_v] - self.vsp) ** 2) / _p.num_nodes

    def cost_grad(self, free, _p):
        g = np.zeros_like(free)
        g[_p._slice_v] = _p.obj_scale / _p.num_nodes * 2 * (free[_p._slice_v] - self.vsp)
        return g


class CostBank:
    """Mean (default) or max squared bank (src/d2d/opty_utils.py:68-82)."""
    use_mean = True

    def cost(self, free, _p):
        sq = free[_p._slice_phi] ** 2
        return _p.obj_scale * (np.sum(sq) / _p.num_nodes if self.use_mean else np.max(sq))

    def cost_grad(self, free, _p):
        g = np.zeros_like(free)
        ph = free[_p._slice_phi]
        if self.use_mean:
            g[_p._slice_phi] = _p.obj_scale / _p.num_nodes * 2 * ph
        else:
            i = np.argmax(ph ** 2)
            g[_p._slice_phi][i] = _p.obj_scale * 2 * ph[i]
        return g


class CostInput:
    """s * (kv sum (v-vsp)^2 + kphi sum phi^2)  (src/d2d/opty_utils.py:85-97)."""

    def __init__(self, vsp=10., kvel=1., kbank=1.):
        self.vsp, self.kv, self.kphi = vsp, kvel, kbank

    def cost(self, free, _p):
        return _p.obj_scale / _p.num_nodes * (self.kv * np.sum((free[_p._slice_v] - self.vsp) ** 2)
                                              + self.kphi * np.sum(free[_p._slice_phi] ** 2))

    def cost_grad(self, free, _p):
        g = np.zeros_like(free)
        g[_p._slice_phi] = self.kphi * 2 * free[_p._slice_phi]
        g[_p._slice_v] = self.kv * 2 * (free[_p._slice_v] - self.vsp)
        return g * (_p.obj_scale / _p.num_nodes)


class CostDuration:
    """k * duration of the plan, for a Problem whose node interval is free (opty's variable duration: the interval is the LAST
    entry of the free vector, duration = (num_nodes - 1) * interval).  cost_grad is zero on the node variables and k (num_nodes - 1)
    on the interval entry.  On a free vector without that entry (a fixed interval) the value is k * the planner's duration and the
    gradient is zero."""

    def __init__(self, k=1.):
        self.k = k

    def cost(self, free, _p):
        n = _p.num_nodes
        return self.k * (n - 1) * (free[-1] if len(free) == 5 * n + 1 else _p.time_step)

    def cost_grad(self, free, _p):
        g = np.zeros_like(free)
        if len(free) == 5 * _p.num_nodes + 1:
            g[-1] = self.k * (_p.num_nodes - 1)
        return g


def _obstacle_field(dx, dy, r, kind, k):
    if kind == 0:
        return np.clip(np.exp(r ** 2 - (dx ** 2 + dy ** 2)), 0., 1e3)
    return np.exp(-((dx / r * k) ** 2 + (dy / r * k) ** 2))


class CostObstacle:
    """Circular obstacle penalty, kind 0 (sharp) or 1 (Gaussian, k=2)  (src/d2d/opty_utils.py:99-134)."""

    def __init__(self, c=(30, 0), r=15., kind=0):
        self.c, self.r, self.kind, self.k = c, r, kind, 2.

    def _d(self, free, _p):
        return free[_p._slice_x] - self.c[0], free[_p._slice_y] - self.c[1]

    def cost1(self, free, _p):
        return _obstacle_field(*self._d(free, _p), self.r, self.kind, self.k)

    def cost(self, free, _p):
        return _p.obj_scale / _p.num_nodes * np.sum(self.cost1(free, _p))

    def cost_grad(self, free, _p):
        dx, dy = self._d(free, _p)
        e = _obstacle_field(dx, dy, self.r, self.kind, self.k)
        g = np.zeros_like(free)
        g[_p._slice_x] = _p.obj_scale / _p.num_nodes * -2. * dx * e      # reference's expression (:131-132)
        g[_p._slice_y] = _p.obj_scale / _p.num_nodes * -2. * dy * e
        return g


class CostObstacles:
    def __init__(self, obss, kind=0):
        self.obss = [CostObstacle(c=(o[0], o[1]), r=o[2], kind=kind) for o in obss]

    def cost(self, free, _p):
        return np.sum([c.cost(free, _p) for c in self.obss])

    def cost_grad(self, free, _p):
        return np.sum([c.cost_grad(free, _p) for c in self.obss], axis=0)


class CostComposit:
    """kobs * obstacles + kvel * air speed + kbank * bank (src/d2d/opty_utils.py:147-165);
    obss=None leaves the obstacle term out, as the reference's try/except does.  kdur (not in the reference): + kdur * duration, for a
    Problem whose node interval is free (CostDuration); without it the class is the reference's."""

    def __init__(self, obss, vsp=10., kobs=1., kvel=1., kbank=1., obs_kind=0, kdur=None):
        self.kobs, self.kvel, self.kbank = kobs, kvel, kbank
        if kdur is not None:
            self.kdur, self.cdur = float(kdur), CostDuration(1.)
        if obss is not None:
            self.cobs = CostObstacles(obss, obs_kind)
        self.cvel = CostAirVel(vsp)
        self.cbank = CostBank()

    def _terms(self):
        t = [(self.kvel, self.cvel), (self.kbank, self.cbank)]
        if hasattr(self, 'cobs'):
            t.insert(0, (self.kobs, self.cobs))
        if hasattr(self, 'cdur'):
            t.append((self.kdur, self.cdur))
        return t

    def cost(self, free, _p):
        return sum(k * c.cost(free, _p) for k, c in self._terms())

    def cost_grad(self, free, _p):
        return sum(k * c.cost_grad(free, _p) for k, c in self._terms())


def triangle(p0, p1, va, duration, num_nodes, go_left=1.):
    """Dog-leg initial guess of length va*duration (src/d2d/opty_utils.py:171-187) -> x, y, psi, phi, v."""
    p0, p1 = np.asarray(p0, dtype=float), np.asarray(p1, dtype=float)
    leg = p1 - p0
    d = np.linalg.norm(leg)
    nrm = np.array([-leg[1], leg[0]]) / d
    D = va * duration
    apex = p0 + leg / 2
    if D > d:
        apex = apex + np.sign(go_left) * np.sqrt(D ** 2 - d ** 2) / 2 * nrm
    n1 = int(num_nodes / 2); n2 = num_nodes - n1
    pts = np.vstack((np.linspace(p0, apex, n1), np.linspace(apex, p1, n2)))
    h0, h1 = apex - p0, p1 - apex
    psis = np.hstack((np.arctan2(h0[1], h0[0]) * np.ones(n1), np.arctan2(h1[1], h1[0]) * np.ones(n2)))
    return pts[:, 0], pts[:, 1], psis, np.zeros(num_nodes), va * np.ones(num_nodes)


class MovingObstacle:
    """A CostObstacle disc whose centre is piecewise linear in time (include/d2d.h d2d_moving_obstacles): knot times t (n,), strictly
    increasing, centres xy (n, 2), radius r, kind 0 / 1 as CostObstacle's.  Between two knots the centre is interpolated linearly;
    before the first and after the last it is held.  Times are absolute, on the clock of the scenario's t0 and of a wind field.
    Scenarios list them in `moving_obstacles`; the collocation backend plans around them with the cost's kobs as their weight."""

    def __init__(self, t, xy, r, kind=1):
        self.t = np.asarray(t, dtype=np.float64).reshape(-1)
        self.xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        self.r, self.kind = float(r), int(kind)
        if len(self.t) < 2 or len(self.t) != len(self.xy):
            raise ValueError('a moving obstacle needs at least two knots, one centre per knot time')
        if not (np.isfinite(self.t).all() and np.isfinite(self.xy).all()):
            raise ValueError('moving obstacle: knot times and centres must be finite')
        if not (np.diff(self.t) > 0).all():
            raise ValueError('moving obstacle: knot times must increase strictly')
        if self.kind not in (0, 1):
            raise ValueError('moving obstacle: kind is 0 or 1 (CostObstacle)')

    @classmethod
    def linear(cls, c0, v, r, t0=0., t1=60., kind=1):
        """A disc at c0 at time t0 that moves with the constant velocity v until t1 (and stands still outside [t0, t1])."""
        c0, v = np.asarray(c0, dtype=np.float64), np.asarray(v, dtype=np.float64)
        return cls((t0, t1), (c0, c0 + v * (t1 - t0)), r, kind)

    def at(self, t):
        """Centres at the times t -> (..., 2): the numpy twin of the device sampler (csrc/nlp_kernels.hip nlp_mov_sample_kernel) --
        the same segment, the same expression up to the device's fused multiply-add."""
        return track_at(self.t, self.xy, t)

    def padded(self, n_knot):
        """(n_knot, 3) rows (t, x, y): the knots, then the last one repeated at strictly later times -- which changes no centre."""
        n = len(self.t)
        if n > n_knot:
            raise ValueError(f'{n} knots do not fit {n_knot}')
        out = np.empty((n_knot, 3))
        out[:n, 0], out[:n, 1:] = self.t, self.xy
        step = max(1.0, abs(self.t[-1]))          # (large enough to be a strict increase at any magnitude of the last time)
        out[n:, 0] = self.t[-1] + step * np.arange(1, n_knot - n + 1)
        out[n:, 1:] = self.xy[-1]
        return out


def track_at(tk, xy, t):
    """Centre of a piecewise-linear track (knot times tk (n,), centres xy (n, 2)) at the times t: linear inside the segment that holds
    t, the first or last knot outside the knots, and a segment's end knot exactly at its end."""
    tk, xy, t = np.asarray(tk, dtype=np.float64), np.asarray(xy, dtype=np.float64), np.asarray(t, dtype=np.float64)
    k = np.clip(np.searchsorted(tk, t, side='right') - 1, 0, len(tk) - 2)
    u = np.maximum((t - tk[k]) / (tk[k + 1] - tk[k]), 0.0)[..., None]
    return np.where(u >= 1.0, xy[k + 1], xy[k] + u * (xy[k + 1] - xy[k]))


def lower_moving(obstacles, n_knot=None):
    """The tables of d2d_moving_obstacles for one problem or scenario: knots (n_mov, n_knot, 3) = (t, x, y) and disc (n_mov, 2) =
    (r, kind).  n_knot: the call's knot count (default: the longest track's); shorter tracks are padded (MovingObstacle.padded).
    NotImplementedError beyond d2dhip.MAX_MOV discs, ValueError beyond d2dhip.MOV_MAX_KNOT knots."""
    import d2dhip
    obstacles = list(obstacles)
    if len(obstacles) > d2dhip.MAX_MOV:
        raise NotImplementedError(f'at most {d2dhip.MAX_MOV} moving obstacles per problem in this build ({len(obstacles)} given)')
    need = max([len(o.t) for o in obstacles], default=2)
    n_knot = need if n_knot is None else int(n_knot)
    if need > d2dhip.MOV_MAX_KNOT or n_knot > d2dhip.MOV_MAX_KNOT:
        raise ValueError(f'at most {d2dhip.MOV_MAX_KNOT} knots per moving obstacle ({max(need, n_knot)} asked for)')
    knots = np.stack([o.padded(n_knot) for o in obstacles]) if obstacles else np.zeros((0, n_knot, 3))
    disc = np.array([(o.r, o.kind) for o in obstacles], dtype=np.float64).reshape(-1, 2)
    return knots, disc


def min_clearance(obstacles, t, x, y):
    """Per moving obstacle: min_i |p_i - c(t_i)| - r over the nodes (t_i, x_i, y_i) of a plan."""
    return [float((np.hypot(*(np.stack([x, y], -1) - o.at(t)).T)).min() - o.r) for o in obstacles]


class KeepOut:
    """A HARD keep-out disc of the collocation planner (include/d2d.h d2d_keep_out): no point of the plan's polyline comes closer
    than `margin` to the disc of radius r round c.  Scenarios list them in `keep_out`; unlike a CostObstacle this is a constraint the
    plan holds, not a price it pays.  The solver holds |p_i - c|^2 >= R^2 at the nodes; lowered() inflates R for the chords between them,
    for nodes at most v_max h apart.  The planners pass the upper AIRSPEED bound as v_max, and the spacing is h times the GROUND speed:
    where a tail wind or a field of speed w can carry the aircraft faster than that bound, the polyline's margin is only guaranteed
    for the smaller value sqrt(R^2 - ((v_max + w) h / 2)^2) - r -- ask for a `margin` larger by the difference (w h / 2 is enough once r + margin >= v_max h / 2)."""

    def __init__(self, c, r, margin=0.0):
        self.c = (float(c[0]), float(c[1]))
        self.r, self.margin = float(r), float(margin)
        if not (np.isfinite(self.c).all() and np.isfinite(self.r) and np.isfinite(self.margin)) or not self.r > 0.0 or not self.margin >= 0.0:
            raise ValueError(f'KeepOut: a finite centre, r > 0 and margin >= 0 are required, got c = {self.c}, r = {self.r}, margin = {self.margin}')

    def lowered(self, v_max, h):
        """(cx, cy, R) of the node constraint: two nodes on the circle R at the largest spacing v_max h have their chord pass the centre
        at sqrt(R^2 - (v_max h / 2)^2) = r + margin.  v_max: the largest speed over the ground, which the planners take to be the upper
        airspeed bound (the class docstring says what a tail wind asks for).  With a FREE time step (t1_window, plan_batch(window=),
        d2d_nlp_solve_free_fence) h is the LARGEST step of the box, h_hi: the chord term grows with h, so the radius lowered with h_hi is
        conservative for every step the solver may end at."""
        return self.c[0], self.c[1], float(np.sqrt((self.r + self.margin) ** 2 + (0.5 * v_max * h) ** 2))

    def __repr__(self):
        return f'KeepOut(c={self.c}, r={self.r}, margin={self.margin})'


def lower_keep_out(keep_out, v_max, h):
    """The rows (n, 3) = (cx, cy, R) of d2d_keep_out for one problem.  NotImplementedError beyond d2dhip.MAX_KEEP discs."""
    import d2dhip
    keep_out = list(keep_out)
    if len(keep_out) > d2dhip.MAX_KEEP:
        raise NotImplementedError(f'at most {d2dhip.MAX_KEEP} keep-out discs per problem in this build ({len(keep_out)} given)')
    return np.array([k.lowered(v_max, h) for k in keep_out], dtype=np.float64).reshape(-1, 3)


def keep_out_clearance(keep_out, x, y):
    """Per keep-out disc: the smallest |p - c| - r over the POLYLINE through the plan's nodes (x_i, y_i)."""
    p = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)], -1)
    a, ab = p[:-1], p[1:] - p[:-1]
    out = []
    for k in keep_out:
        c = np.asarray(k.c)
        t = np.clip(np.sum((c - a) * ab, 1) / np.maximum(np.sum(ab * ab, 1), 1e-300), 0.0, 1.0)
        out.append(float(np.hypot(*(a + t[:, None] * ab - c).T).min() - k.r))
    return out


class MovingKeepOut:
    """A HARD keep-out disc that moves (include/d2d.h d2d_nlp_solve_keepout_moving): no point of the plan comes closer than `margin` to
    the disc of radius r round the piecewise-linear track (t, xy) -- knots as MovingObstacle's, validated alike, times absolute.
    Scenarios list them in `keep_out`, beside static KeepOut discs.  The solver holds |p_i - c(t_i)|^2 >= R^2 at the nodes; lowered()
    inflates R for what happens between them: between two nodes the RELATIVE displacement of aircraft and disc is what cuts the chord,
    at most (v_max + v_c) h with v_c the track's fastest knot segment."""

    def __init__(self, t, xy, r, margin=0.0):
        trk = MovingObstacle(t, xy, r, kind=1)       # (the track's checks are MovingObstacle's)
        self.t, self.xy, self.r, self.margin = trk.t, trk.xy, float(r), float(margin)
        if not (np.isfinite(self.r) and np.isfinite(self.margin)) or not self.r > 0.0 or not self.margin >= 0.0:
            raise ValueError(f'MovingKeepOut: r > 0 and margin >= 0 are required, got r = {self.r}, margin = {self.margin}')

    @classmethod
    def linear(cls, c0, v, r, t0=0., t1=60., margin=0.0):
        c0, v = np.asarray(c0, dtype=np.float64), np.asarray(v, dtype=np.float64)
        return cls((t0, t1), (c0, c0 + v * (t1 - t0)), r, margin)

    def at(self, t):
        return track_at(self.t, self.xy, t)

    @property
    def v_c(self):
        """the track's fastest knot segment (m/s)"""
        return float((np.hypot(*np.diff(self.xy, axis=0).T) / np.diff(self.t)).max())

    def lowered(self, v_max, h):
        """R of the node constraint: two nodes whose relative positions lie on the circle R and differ by at most s = (v_max + v_c) h
        have their relative chord pass the centre at sqrt(R^2 - (s / 2)^2) = r + margin."""
        return float(np.sqrt((self.r + self.margin) ** 2 + (0.5 * (v_max + self.v_c) * h) ** 2))

    def track(self, v_max, h):
        """The MovingObstacle whose table row the kernel reads: the track with the node radius in the place of r."""
        return MovingObstacle(self.t, self.xy, self.lowered(v_max, h), kind=1)

    def __repr__(self):
        return f'MovingKeepOut({len(self.t)} knots, r={self.r}, margin={self.margin})'


def lower_keep_moving(keep_out, v_max, h, n_knot=None):
    """The tables of d2d_nlp_solve_keepout_moving for one problem: knots (n, n_knot, 3) and disc (n, 2) = (R, 1) of a list of
    MovingKeepOut and KeepOut -- a static disc lowers to a two-knot track that stands still (its R is KeepOut.lowered's)."""
    trk = []
    for k in keep_out:
        if isinstance(k, MovingKeepOut):
            trk.append(k.track(v_max, h))
        else:
            cx, cy, R = k.lowered(v_max, h)
            trk.append(MovingObstacle((0.0, 1.0), ((cx, cy), (cx, cy)), R, kind=1))
    return lower_moving(trk, n_knot)


def moving_keep_clearance(keep_out, t, x, y):
    """Per disc of a keep_out list (MovingKeepOut or KeepOut): the smallest |p(t) - c(t)| - r, continuous in time, over the plan's
    polyline (t_i, x_i, y_i) -- the relative position is taken piecewise linear between the plan's nodes and the track's knots."""
    t, x, y = (np.asarray(v, dtype=np.float64) for v in (t, x, y))
    out = []
    for k in keep_out:
        if not isinstance(k, MovingKeepOut):
            out.append(keep_out_clearance([k], x, y)[0])
            continue
        tt = np.union1d(t, k.t[(k.t > t[0]) & (k.t < t[-1])])
        d = np.stack([np.interp(tt, t, x), np.interp(tt, t, y)], -1) - k.at(tt)
        a, ab = d[:-1], d[1:] - d[:-1]
        s = np.clip(-np.sum(a * ab, 1) / np.maximum(np.sum(ab * ab, 1), 1e-300), 0.0, 1.0)
        out.append(float(np.hypot(*(a + s[:, None] * ab).T).min() - k.r))
    return out


class GeoFence:
    """A HARD geofence of the collocation planner (include/d2d.h d2d_fence): every point of the plan's polyline stays inside the strictly
    convex polygon `vertices` (3 to 8 of them, either orientation), at least `margin` from every edge.  Scenarios carry one in `fence`.
    The solver holds b_k - a_k . p_i > 0 at the nodes, with a_k edge k's outward unit normal; the half-planes' intersection is convex, so
    the segment between two nodes that hold them holds them too -- unlike a KeepOut, nothing is inflated for the chords."""

    MAX_VERTICES = 8                        # include/d2d.h D2D_MAX_FENCE

    def __init__(self, vertices, margin=0.0):
        v = np.array(vertices, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 2 or not 3 <= len(v) <= self.MAX_VERTICES or not np.isfinite(v).all():
            raise ValueError(f'GeoFence: 3 to {self.MAX_VERTICES} finite vertices (x, y) are required, got an array of shape {v.shape}')
        n = len(v)
        e = np.roll(v, -1, axis=0) - v                                   # edge k: vertex k -> vertex k + 1
        ln = np.hypot(e[:, 0], e[:, 1])
        for k in range(n):
            if not ln[k] > 0.0:
                raise ValueError(f'GeoFence: vertex {(k + 1) % n} repeats vertex {k}')
        ein = np.roll(e, 1, axis=0); lin = np.roll(ln, 1)                # the edge that ARRIVES at vertex k
        cr = ein[:, 0] * e[:, 1] - ein[:, 1] * e[:, 0]                   # the turn at vertex k
        for k in range(n):
            if abs(cr[k]) <= 1e-12 * lin[k] * ln[k]:
                raise ValueError(f'GeoFence: vertex {k} is collinear with its neighbours')
        sg = 1.0 if float(np.sum(v[:, 0] * np.roll(v[:, 1], -1) - np.roll(v[:, 0], -1) * v[:, 1])) > 0.0 else -1.0     # +1: counter-clockwise
        for k in range(n):
            if cr[k] * sg < 0.0:
                raise ValueError(f'GeoFence: the polygon is not convex at vertex {k}')
        turn = float(np.sum(np.arctan2(cr, np.sum(ein * e, 1))))          # a simple polygon turns once round
        if abs(abs(turn) - 2.0 * np.pi) > 1e-6:
            raise ValueError('GeoFence: the polygon crosses itself (vertex 0 is passed more than once round)')
        self.vertices = v
        self.margin = float(margin)
        if not np.isfinite(self.margin) or not self.margin >= 0.0:
            raise ValueError(f'GeoFence: margin >= 0 is required, got {self.margin}')
        self.a = sg * np.stack([e[:, 1], -e[:, 0]], 1) / ln[:, None]     # outward unit normals
        self.b = np.sum(self.a * v, 1)
        shrunk = self._clip(v if sg > 0 else v[::-1], self.a, self.b - self.margin)
        if len(shrunk) < 3:
            raise ValueError(f'GeoFence: margin = {self.margin} leaves nothing of the polygon')
        # kap_k, where the start rule puts a node that is closer to edge k: 1e-2 of the shrunk polygon's width along a_k
        self.kap = 1e-2 * np.array([float(np.max(self.b[k] - self.margin - shrunk @ self.a[k])) for k in range(n)])
        if not (self.kap > 0.0).all():
            raise ValueError(f'GeoFence: margin = {self.margin} leaves nothing of the polygon')

    @staticmethod
    def _clip(poly, a, b):
        """The counter-clockwise polygon `poly` cut by every half-plane a_k . p <= b_k (Sutherland-Hodgman)."""
        for ak, bk in zip(a, b):
            out = []
            for j in range(len(poly)):
                p, q = poly[j], poly[(j + 1) % len(poly)]
                gp, gq = bk - float(ak @ p), bk - float(ak @ q)
                if gp >= 0.0:
                    out.append(p)
                if (gp > 0.0 and gq < 0.0) or (gp < 0.0 and gq > 0.0):
                    out.append(p + (q - p) * (gp / (gp - gq)))
            poly = np.array(out).reshape(-1, 2)
            if len(poly) < 3:
                break
        return poly

    def lowered(self):
        """The rows (n, 4) = (ax, ay, b - margin, kap) of d2d_fence for one problem."""
        return np.column_stack([self.a, self.b - self.margin, self.kap])

    def __repr__(self):
        return f'GeoFence({len(self.vertices)} vertices, margin={self.margin})'


def lower_fence(fence):
    """The rows (n, 4) of d2d_fence for one problem from a GeoFence (or rows already lowered: checked for their shape and passed on)."""
    if isinstance(fence, GeoFence):
        return fence.lowered()
    rows = np.array(fence, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 4 or len(rows) > GeoFence.MAX_VERTICES:
        raise ValueError(f'fence: a GeoFence or rows (n <= {GeoFence.MAX_VERTICES}, 4) = (ax, ay, b, kap) are required, got shape {rows.shape}')
    return rows


def fence_clearance(fence, x, y):
    """Per edge: the smallest b_k - a_k . p over the plan's nodes (x_i, y_i).  With a GeoFence that is the distance from the USER's polygon
    (margin not taken off): every plan the solver returns has it >= margin, and by convexity so has every point of the polyline between
    the nodes.  With lowered rows (n, 4) -- what plan_batch also takes -- it is the distance from the rows' own half-planes, whose margin
    is already taken off: >= 0 for every returned plan; absent rows (ax = ay = 0) give +inf."""
    p = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)], -1)
    if isinstance(fence, GeoFence):
        a, b = fence.a, fence.b
    else:
        rows = lower_fence(fence)
        a, b = rows[:, :2], np.where((rows[:, 0] != 0.0) | (rows[:, 1] != 0.0), rows[:, 2], np.inf)
    return [float(np.min(b[k] - p @ a[k])) for k in range(len(a))]


class Waypoint:
    """A timed waypoint of the collocation planner (include/d2d.h d2d_via_points): at time t -- absolute, on the clock of the scenario's
    t0 -- the given ones of x, y, psi hold exactly; None leaves a component free.  The time must be that of an interior node of the
    plan (lower_waypoints).  Scenarios list them in `waypoints`: one list for single_opt_planner, one list per aircraft for
    multi_opt_planner."""

    def __init__(self, t, x=None, y=None, psi=None):
        self.t = float(t)
        self.x, self.y, self.psi = (None if v is None else float(v) for v in (x, y, psi))
        if self.x is None and self.y is None and self.psi is None:
            raise ValueError('a waypoint pins at least one of x, y, psi')
        if not np.isfinite([self.t] + [v for v in (self.x, self.y, self.psi) if v is not None]).all():
            raise ValueError('waypoint: time and pinned values must be finite')

    @property
    def mask(self):
        """bit 0 / 1 / 2: x / y / psi is pinned"""
        return (self.x is not None) * 1 + (self.y is not None) * 2 + (self.psi is not None) * 4

    def __repr__(self):
        return f'Waypoint(t={self.t}, x={self.x}, y={self.y}, psi={self.psi})'


def waypoint_node(t, t_start, h, N):
    """The node of the time t on the grid t_start + k h, k = 0 .. N-1.  ValueError (naming the two nearest node times) when t is on
    no node, and when it is on the first or last one: those carry the end conditions."""
    k = int(round((t - t_start) / h))
    if abs(t - (t_start + k * h)) > 1e-9 * max(1.0, abs(t)):
        k0 = int(np.floor((t - t_start) / h))
        raise ValueError(f'waypoint time {t} is not a node time: the nearest nodes are at {t_start + k0 * h} and {t_start + (k0 + 1) * h} '
                         f'(t0 = {t_start}, time step {h})')
    if k <= 0 or k >= N - 1:
        if k == 0 or k == N - 1:
            raise ValueError(f'waypoint time {t} is the {"first" if k == 0 else "last"} node: x, y, psi there are the end conditions (p0 / p1)')
        raise ValueError(f'waypoint time {t} lies outside the plan [{t_start}, {t_start + (N - 1) * h}]')
    return k


def lower_waypoints(waypoints, t_start, h, N, n_via=None):
    """The table of d2d_via_points for one problem: (n_via, 5) rows (node, mask, x, y, psi), a free component 0.  n_via: the call's row
    count (default: the list's length); shorter lists are padded with rows of mask 0, which the kernels skip.  ValueError for a time
    that is no interior node (waypoint_node), a (node, component) pinned twice, or more than d2dhip.MAX_VIA rows."""
    import d2dhip
    waypoints = list(waypoints or [])
    n_via = len(waypoints) if n_via is None else int(n_via)
    if len(waypoints) > d2dhip.MAX_VIA or n_via > d2dhip.MAX_VIA:
        raise ValueError(f'at most {d2dhip.MAX_VIA} waypoints per problem ({max(len(waypoints), n_via)} asked for)')
    if len(waypoints) > n_via:
        raise ValueError(f'{len(waypoints)} waypoints do not fit {n_via} rows')
    out = np.zeros((n_via, 5))
    seen = {}
    for e, w in enumerate(waypoints):
        k = waypoint_node(w.t, t_start, h, N)
        if seen.get(k, 0) & w.mask:
            raise ValueError(f'two waypoints pin the same component at time {w.t} (node {k})')
        seen[k] = seen.get(k, 0) | w.mask
        out[e] = (k, w.mask, w.x or 0.0, w.y or 0.0, w.psi or 0.0)
    return out


def via_guess(p0, p1, waypoints, t_start, h, N, vref):
    """Piecewise-linear guess through p0, the waypoints that pin both x and y (in time order) and p1 -> x, y, psi, phi, v: positions
    linear in time on every leg, psi along the leg, phi = 0, v = vref."""
    pts = [(0, float(p0[0]), float(p0[1]))]
    for w in sorted(waypoints or [], key=lambda w: w.t):
        if w.x is not None and w.y is not None:
            pts.append((waypoint_node(w.t, t_start, h, N), w.x, w.y))
    pts.append((N - 1, float(p1[0]), float(p1[1])))
    kk, xx, yy = (np.array(v, dtype=np.float64) for v in zip(*pts))
    i = np.arange(N, dtype=np.float64)
    x, y = np.interp(i, kk, xx), np.interp(i, kk, yy)
    leg = np.clip(np.searchsorted(kk, i, side='right') - 1, 0, len(kk) - 2)
    psi = np.arctan2(yy[leg + 1] - yy[leg], xx[leg + 1] - xx[leg])
    return x, y, psi, np.zeros(N), vref * np.ones(N)


def waypoint_error(table, W):
    """Largest |plan - pin| over the rows of a d2d_via_points table (n_via, 5) and a plan W (5, N)."""
    err = 0.0
    for node, mask, *val in np.asarray(table, dtype=np.float64):
        for c in range(3):
            if (int(mask) >> c) & 1:
                err = max(err, abs(float(W[c][int(node)]) - val[c]))
    return err
