"""Which collocation entry the planners call, and with what: tests/golden/nlp_dispatch_parent.json.

    python tests/golden/make_nlp_dispatch_golden.py        (no GPU, no built library)

d2dhip.default_context is replaced by a recording stand-in: dev() keeps tensors on the CPU, sync() does nothing, and every nlp_solve*
method binds its arguments to the signature of the real d2dhip.Context method (so a keyword and a positional argument record alike),
records its name, the SHA-256 of every tensor argument's bytes and the scalars, and returns canned outputs of the right shapes (W
untouched, status 1, zeros; the solved step of nlp_solve_free: the start step).  Nothing is solved: what is recorded is the routing --
the entry, the rows, the tables and the options -- of the ladders a stand-in can reach: opty.direct_collocation.Problem.solve through
both planners and full_sim.plan_batch.  The committed file was written by this script at the commit BEFORE the planners' ladders were
folded into d2dhip.nlp_plan; tests/test_nlp_dispatch_cpu.py replays collect() and asserts equality call by call."""
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(ROOT, 'tests', 'golden', 'nlp_dispatch_parent.json')

import d2dhip                                   # noqa: E402
import d2d.multiopty_utils as d2mou             # noqa: E402
import d2d.opty_utils as d2ou                   # noqa: E402
from d2d.wind import SplineWindField            # noqa: E402

ENTRIES = ('nlp_solve', 'nlp_solve_free', 'nlp_solve_wind', 'nlp_solve_groups', 'nlp_solve_groups_wind', 'nlp_solve_groups_pairs',
           'nlp_solve_moving', 'nlp_solve_groups_moving', 'nlp_solve_via', 'nlp_solve_groups_via', 'nlp_solve_model')


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _rec(v):
    """A JSON value that identifies an argument: tensors and arrays by shape, dtype and the hash of their bytes."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, np.generic):
        return _rec(v.item())
    if torch.is_tensor(v):
        a = v.detach().cpu().contiguous().numpy()
        return {'tensor': list(a.shape), 'dtype': str(a.dtype), 'sha256': _sha(a.tobytes())}
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return {'array': list(a.shape), 'dtype': str(a.dtype), 'sha256': _sha(a.tobytes())}
    if isinstance(v, SplineWindField):
        return {'field': _sha(np.ascontiguousarray(v.cp).tobytes()), 'grid': [repr(float(x)) for x in (v.t0, v.ht, v.x0, v.hx, v.y0, v.hy)]}
    if isinstance(v, (tuple, list)):
        return [_rec(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _rec(x) for k, x in sorted(v.items())}
    raise TypeError(f'cannot record a {type(v).__name__}')


class RecordingContext:
    """Stands where d2dhip.default_context() returns the process's Context: CPU tensors, recorded nlp_solve* calls."""

    def __init__(self):
        self.calls = []
        self.device = torch.device('cpu')

    def dev(self, a, dtype=None):
        t = a.clone() if torch.is_tensor(a) else torch.from_numpy(np.array(a))        # (a copy, as an upload is)
        return (t if dtype is None else t.to(dtype)).contiguous()

    def sync(self):
        pass

    def _solve(self, name, *a, **kw):
        b = inspect.signature(getattr(d2dhip.Context, name)).bind(self, *a, **kw)
        b.apply_defaults()
        args = {k: v for k, v in b.arguments.items() if k != 'self'}
        self.calls.append({'entry': name, 'args': {k: _rec(v) for k, v in args.items()}})
        W, h, n_ac = args['W'], args['h'], args.get('n_ac')
        B, _, N = W.shape
        G = B // n_ac if n_ac else B
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                            # noqa: E731
        out = dict(cost=torch.zeros(B, dtype=torch.float64), feas=torch.zeros(B, dtype=torch.float64), iters=i32(B), status=i32(B) + 1,
                   work=None, mult=torch.zeros(B, 3, N, dtype=torch.float64))
        if n_ac:
            out.update(sweeps=i32(G), moved=torch.zeros(G, dtype=torch.float64), prev=torch.zeros(G, 2, N, dtype=torch.float64))
        if name == 'nlp_solve_free':
            out['h'] = torch.full((B,), float(h), dtype=torch.float64)
        if 'knots' in args:
            n_mov = 0 if args['knots'] is None else args['knots'].shape[1]
            out['mov_work'] = torch.zeros(G, n_mov, 2, N, dtype=torch.float64) if n_mov else None
            out['t_start'] = args.get('t_start')
        if 'via' in args:
            out['via_work'] = None if args['via'] is None else i32(B, N)
        return out


for _name in ENTRIES:
    setattr(RecordingContext, _name, (lambda name: lambda self, *a, **kw: self._solve(name, *a, **kw))(_name))


def _field():
    """A small field that varies in time and space (4 x 5 x 6 control points per component)."""
    t, y, x = np.meshgrid(np.arange(4.0), np.arange(5.0), np.arange(6.0), indexing='ij')
    cp = np.stack([1.0 + 0.3 * x - 0.2 * y + 0.5 * t, -0.5 + 0.1 * x * y - 0.25 * t], axis=1)        # (nt, 2, ny, nx)
    return SplineWindField(cp, -200.0, 100.0, -200.0, 120.0, t0=-10.0, ht=40.0)


def _disc(t1):
    return d2ou.MovingObstacle((-5.0, t1 + 5.0), ((20.0, -30.0), (25.0, 30.0)), 6.0, kind=1)


def _single_scenarios():
    import single_opt_planner as sop

    class base(sop.exp_1):                       # 9 nodes
        p0 = (0., 0., 0., 0., 12.)
        t0, t1, hz, p1 = 0., 4., 2, (45., 6., 0.1, 0., 12.)
        cost = d2ou.CostComposit([(20., 9., 4.)], vsp=12., kobs=2., kvel=5., kbank=1., obs_kind=1)

    def sub(**kw):
        return type('exp', (base,), kw)

    fld = _field()
    return [('plain', sub()),
            ('phi_asymmetric', sub(phi_constraint=(-np.deg2rad(25.), np.deg2rad(40.)))),
            ('field', sub(wind=fld)),
            ('moving_disc', sub(moving_obstacles=[_disc(4.)])),
            ('waypoint', sub(waypoints=[d2ou.Waypoint(2.0, 22.0, 5.0)])),
            ('waypoint_disc_field', sub(waypoints=[d2ou.Waypoint(3.5, psi=0.05)], moving_obstacles=[_disc(4.)], wind=fld, t0=2.0, t1=6.0)),
            ('t1_free', sub(t1_free=(3.0, 7.0), cost=d2ou.CostComposit(None, vsp=12., kvel=5., kbank=1., kdur=0.3)))]


def _multi_scenarios():
    import multi_opt_planner as mop
    nan = float('nan')

    def comp(kcol, **kw):
        return d2mou.CostComposit(kvel=70., kbank=1., kobs=nan, kcol=kcol, vsp=12., obss=[], obs_kind=0, rcol=10., **kw)

    class two(mop.trap_4):                       # 11 nodes
        t0, t1, hz = 0., 5., 2
        p0s = ((0., 0., 0., 0., 12.), (0., 40., 0., 0., 12.)); p1s = ((60., 40., 0., 0., 12.), (60., 0., 0., 0., 12.))
        cost = comp(10.)

    p3 = ((0., 0., 0., 0., 12.), (0., 40., 0., 0., 12.), (0., 80., 0., 0., 12.))
    q3 = ((60., 80., 0., 0., 12.), (60., 40., 0., 0., 12.), (60., 0., 0., 0., 12.))
    wps = [[d2ou.Waypoint(2.5, 30.0, 18.0)], []]
    sub = lambda **kw: type('scen', (two,), kw)                                        # noqa: E731
    return [('one_aircraft', sub(p0s=two.p0s[:1], p1s=two.p1s[:1], cost=comp(nan))),
            ('two_default_pair', two),
            ('two_uncoupled', sub(cost=comp(nan))),
            ('three_pairs', sub(p0s=p3, p1s=q3, cost=comp(10., col_pairs=[(0, 2), (1, 2)]))),
            ('three_pairs_all_obstacle', sub(p0s=p3, p1s=q3, cost=d2mou.CostComposit(kvel=70., kbank=1., kobs=3., kcol=10., vsp=12.,
                                                                                     obss=[(30., 20., 5.)], obs_kind=1, rcol=10., col_pairs='all'))),
            ('two_discs', sub(moving_obstacles=[_disc(5.)])),
            ('two_waypoints', sub(waypoints=wps)),
            ('two_waypoints_discs', sub(waypoints=wps, moving_obstacles=[_disc(5.)])),
            ('two_uncoupled_waypoints', sub(waypoints=wps, cost=comp(nan))),
            ('three_pairs_discs', sub(p0s=p3, p1s=q3, cost=comp(10., col_pairs=[(0, 1), (1, 2)]), moving_obstacles=[_disc(5.)]))]


def _plan_batch_cases():
    """name -> (rows, n_ac, keyword arguments of plan_batch) over 7 nodes."""
    import multi_opt_planner as mop
    import single_opt_planner as sop
    sop.get_plan = lambda *a, **k: None          # (scenario_rows also returns the fit's plan, which needs the library: not looked at here)
    nan = float('nan')
    N, h = 7, 0.5

    def rows_of(n, kcol=10., **kw):
        class scen(mop.trap_4):
            cost = d2mou.CostComposit(kvel=70., kbank=1., kobs=nan, kcol=kcol, vsp=12., obss=[], obs_kind=0, rcol=10., **kw)
        p0s = [(0., 40. * a, 0., 0., 12.) for a in range(n)]
        p1s = [(36., 40. * (n - 1 - a), 0., 0., 12.) for a in range(n)]
        return mop.scenario_rows(scen, p0s, p1s, N, (N - 1) * h, 1.0, (0.5, -0.25))[0]

    def guess(rows):
        s = np.linspace(0.0, 1.0, N)
        x = rows[:, d2dhip.SC_X0, None] + s * (rows[:, d2dhip.SC_X1] - rows[:, d2dhip.SC_X0])[:, None]
        y = rows[:, d2dhip.SC_Y0, None] + s * (rows[:, d2dhip.SC_Y1] - rows[:, d2dhip.SC_Y0])[:, None]
        z = np.zeros_like(x)
        return np.ascontiguousarray(np.stack([x, y, z, z, z + 12.0], axis=1))

    masked = np.concatenate([rows_of(2), rows_of(2)])                 # two scenarios of the default pair, masks written
    bare = masked.copy(); bare[:, d2dhip.SC_PMASK] = 0.0              # the same rows without masks
    half = bare.copy(); half[2:, d2dhip.SC_KCOL] = 0.0                # ... the second scenario uncoupled
    trio = rows_of(3, col_pairs=[(0, 2), (1, 2)])                     # partner sets other than the default pair's
    solo = np.concatenate([rows_of(1, kcol=nan)] * 3)
    fld = _field()
    disc, discs = [_disc(3.)], [[_disc(3.)], [_disc(4.)]]
    wp, wp_late = d2ou.Waypoint(1.5, 20.0, 4.0), d2ou.Waypoint(4.5, y=3.0)
    ts = torch.tensor([1.0, 2.5], dtype=torch.float64)
    kw = dict(max_sweeps=5, tol=1e-6)
    cases = [('groups_masked', masked, 2, {}), ('groups_bare', bare, 2, kw), ('groups_solo', solo, 1, {}),
             ('wind_float', masked, 2, dict(windfield=fld, t_start=1.5)), ('wind_tensor', bare, 2, dict(windfield=fld, t_start=ts, **kw)),
             ('pairs', trio, 3, {}), ('pairs_wind', trio, 3, dict(windfield=fld, t_start=0.5)),
             ('moving_masked', masked, 2, dict(moving=disc, t_start=1.0)), ('moving_bare', bare, 2, dict(moving=discs, t_start=ts)),
             ('moving_wind', half, 2, dict(moving=disc, windfield=fld, t_start=ts, **kw)), ('moving_pairs', trio, 3, dict(moving=disc)),
             ('moving_solo', solo, 1, dict(moving=disc, t_start=0.0)),
             ('via_masked', masked, 2, dict(via=[[wp], [], [], [wp]])), ('via_bare', bare, 2, dict(via=[[wp], [], [], []], t_start=1.0)),
             ('via_half', half, 2, dict(via=[[wp], [], [wp], []], **kw)), ('via_pairs', trio, 3, dict(via=[[], [wp], []])),
             ('via_solo', solo, 1, dict(via=[[wp], [], [wp]])), ('via_solo_empty', solo, 1, dict(via=[[], [], []])),
             ('via_moving', bare, 2, dict(via=[[wp], [], [], []], moving=discs, t_start=ts)),
             ('via_wind', masked, 2, dict(via=[[wp], [], [], []], windfield=fld, t_start=ts)),
             ('via_moving_wind', half, 2, dict(via=[[d2ou.Waypoint(3.0, psi=0.1)], [], [], [wp_late]], moving=disc, windfield=fld, t_start=2.0)),
             ('free_scalar', solo, 1, dict(free_time=(0.25, 1.0), kdur=0.4)),
             ('free_rows', solo, 1, dict(free_time=np.array([[0.25, 1.0], [0.3, 0.9], [0.4, 0.8]]), kdur=np.array([0.0, 0.2, 0.4]),
                                         opt_tol=1e-6))]
    return N, h, guess, cases


def collect():
    """{configuration: {'calls': [...], ...}} of every configuration, with the recording stand-in as the default context."""
    import full_sim as fs
    import multi_opt_planner as mop
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    real = d2dhip.default_context
    real_plan = sop.get_plan
    ctx = RecordingContext()
    d2dhip.default_context = lambda: ctx
    out = {}

    def take(name, **extra):
        out[name] = dict(calls=ctx.calls, **extra)
        ctx.calls = []

    try:
        for name, exp in _single_scenarios():
            p = sop.Planner(exp, backend='nlp')
            p.configure(tol=1e-6, max_iter=900)
            p.run()
            take('single/' + name, info=sorted(p.info), backend_used=p.info.get('backend_used'))
        # a psi box and an asymmetric phi interval, as a caller of opty's Problem spells them
        exp = _single_scenarios()[0][1]
        p = sop.Planner(exp, backend='nlp')
        g = p.aircraft
        bounds = dict(p._bounds)
        bounds[g._spsi(g._st)] = (-1.0, 1.5)
        prob = odc.Problem(p.prob.obj, p.prob.obj_grad, g.get_eom(p.wind), g._state_symbols, p.num_nodes, p.time_step, known_parameter_map={},
                           instance_constraints=p._instance_constraints, bounds=bounds)
        prob.addOption('max_sweeps', 7)
        _, info = prob.solve(p.get_initial_guess())
        take('single/psi_box', info=sorted(info))
        # backend='auto': the fit's plan (here: the guess) overshoots a bound -> the hardening call
        p = sop.Planner(exp, initialize=False, backend='auto')
        p.prob = sop._FitProblem(p, 1)
        p.prob.addOption('tol', 1e-5)
        p.solution, p.info = sop.Planner(exp, backend='nlp').get_initial_guess(), {'phi_violation': 0.1}
        p._harden()
        take('single/auto_harden', info=sorted(p.info), backend_used=p.info.get('backend_used'))
        for name, scen in _multi_scenarios():
            m = mop.Planner(scen, backend='nlp')
            m.run(tol=1e-6, max_iter=700)
            take('multi/' + name, info=sorted(m.info), backend_used=m.info.get('backend_used'))
        N, h, guess, cases = _plan_batch_cases()
        for name, rows, n_ac, kw in cases:
            res = fs.plan_batch(rows.copy(), N, (N - 1) * h, 1.0 / N, backend='nlp', W0=guess(rows), h=h, n_ac=n_ac, **kw)
            take('plan_batch/' + name, scen=_rec(res['scen']), keys=sorted(k for k in res if k != 'entry'))
    finally:
        d2dhip.default_context = real
        sop.get_plan = real_plan
    return out


if __name__ == '__main__':
    res = collect()
    with open(OUT, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{OUT}: {len(res)} configurations, {sum(len(v["calls"]) for v in res.values())} calls')
