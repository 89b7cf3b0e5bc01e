"""Which collocation entry the planners call, and with what: tests/golden/nlp_dispatch_parent.json.

    python tests/golden/make_nlp_dispatch_golden.py        (no GPU, no built library)

d2dhip.default_context is replaced by a recording stand-in: dev() keeps tensors on the CPU, sync() does nothing, and every nlp_solve*
method binds its arguments to the signature of the real d2dhip.Context method (so a keyword and a positional argument record alike),
records its name, the SHA-256 of every tensor argument's bytes and the scalars, and returns canned outputs of the right shapes (W
untouched, status 1, zeros; the solved step of nlp_solve_free: the start step).  Nothing is solved: what is recorded is the routing --
the entry, the rows, the tables and the options -- of the ladders a stand-in can reach: opty.direct_collocation.Problem.solve through
both planners and full_sim.plan_batch.  The committed file was written by this script at the commit BEFORE the planners' ladders were
folded into d2dhip.nlp_plan; tests/test_nlp_dispatch_cpu.py replays collect() and asserts equality call by call.

Two more files were written by this script at the commit BEFORE nlp_plan and plan_batch were restated as tables:
  nlp_dispatch_abi129.json     collect('abi129'): the accepted calls of the six entries added since -- hard discs, hard moving discs,
                               the geofence, the free step beside them -- and of deconflict= and W0='dubins';
  nlp_dispatch_refusals.json   refusals(): the outcome of nlp_plan for every subset of its 13 optional inputs (8192 calls on a stub)
                               and of plan_batch for backend x n_ac x every subset of its 10 optional features (4096 calls on the
                               stand-in) -- the entry reached and what it was handed, or the exception's type and full text -- as the
                               distinct outcomes and one index per subset.
    python tests/golden/make_nlp_dispatch_golden.py abi129 | refusals"""
import hashlib
import inspect
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLD = os.path.join(ROOT, 'tests', 'golden')

import d2dhip                                   # noqa: E402
import d2d.multiopty_utils as d2mou             # noqa: E402
import d2d.opty_utils as d2ou                   # noqa: E402
from d2d.wind import SplineWindField            # noqa: E402

ENTRIES = ('nlp_solve', 'nlp_solve_free', 'nlp_solve_wind', 'nlp_solve_groups', 'nlp_solve_groups_wind', 'nlp_solve_groups_pairs',
           'nlp_solve_moving', 'nlp_solve_groups_moving', 'nlp_solve_via', 'nlp_solve_groups_via', 'nlp_solve_model',
           'nlp_solve_keepout', 'nlp_solve_fence', 'nlp_solve_free_fence', 'nlp_solve_groups_fence', 'nlp_solve_keepout_moving',
           'nlp_solve_groups_keepout')


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
        if 'free_rows' in args:
            out['h'] = torch.full((B,), float(h), dtype=torch.float64)
        if 'knots' in args:
            n_mov = 0 if args['knots'] is None else args['knots'].shape[1]
            out['mov_work'] = torch.zeros(G, n_mov, 2, N, dtype=torch.float64) if n_mov else None
            out['t_start'] = args.get('t_start')
        if 'via' in args:
            out['via_work'] = None if args['via'] is None else i32(B, N)
        if name in ('nlp_solve_keepout_moving', 'nlp_solve_groups_keepout'):
            out['keep_mult'] = torch.zeros(B, n_mov, N, dtype=torch.float64) if n_mov else None
        if 'discs' in args:
            out['keep_mult'] = None if args['discs'] is None else torch.zeros(B, args['discs'].shape[1], N, dtype=torch.float64)
        if 'edges' in args:
            out['fence_mult'] = None if args['edges'] is None else torch.zeros(B, args['edges'].shape[1], N, dtype=torch.float64)
        return out

    def nlp_guess_dubins(self, scen, N, h, bounds=None, outputs=None):
        self.calls.append({'entry': 'nlp_guess_dubins', 'args': {k: _rec(v) for k, v in dict(scen=scen, N=N, h=h, bounds=bounds, outputs=outputs).items()}})
        B = scen.shape[0]
        return torch.zeros(B, 5, N, dtype=torch.float64), {'status': torch.ones(B, dtype=torch.int32)}


for _name in ENTRIES:
    setattr(RecordingContext, _name, (lambda name: lambda self, *a, **kw: self._solve(name, *a, **kw))(_name))


def _field():
    """A small field that varies in time and space (4 x 5 x 6 control points per component)."""
    t, y, x = np.meshgrid(np.arange(4.0), np.arange(5.0), np.arange(6.0), indexing='ij')
    cp = np.stack([1.0 + 0.3 * x - 0.2 * y + 0.5 * t, -0.5 + 0.1 * x * y - 0.25 * t], axis=1)        # (nt, 2, ny, nx)
    return SplineWindField(cp, -200.0, 100.0, -200.0, 120.0, t0=-10.0, ht=40.0)


def _disc(t1):
    return d2ou.MovingObstacle((-5.0, t1 + 5.0), ((20.0, -30.0), (25.0, 30.0)), 6.0, kind=1)


def _hard(t1):
    return d2ou.MovingKeepOut((-5.0, t1 + 5.0), ((20.0, -60.0), (25.0, -35.0)), 4.0, margin=0.5)


KEEP = d2ou.KeepOut((22.0, 70.0), 5.0, margin=1.0)
FENCE = d2ou.GeoFence([(-60.0, -80.0), (120.0, -80.0), (120.0, 160.0), (-60.0, 160.0)], margin=1.0)


def _single_scenarios(which='parent'):
    import single_opt_planner as sop

    class base(sop.exp_1):                       # 9 nodes
        p0 = (0., 0., 0., 0., 12.)
        t0, t1, hz, p1 = 0., 4., 2, (45., 6., 0.1, 0., 12.)
        cost = d2ou.CostComposit([(20., 9., 4.)], vsp=12., kobs=2., kvel=5., kbank=1., obs_kind=1)

    def sub(**kw):
        return type('exp', (base,), kw)

    fld = _field()
    if which == 'abi129':
        dur = d2ou.CostComposit(None, vsp=12., kvel=5., kbank=1., kdur=0.3)
        return [('keep_out', sub(keep_out=[KEEP])), ('keep_out_field', sub(keep_out=[KEEP], wind=fld, t0=2.0, t1=6.0)),
                ('keep_moving', sub(keep_out=[_hard(4.), KEEP])), ('fence', sub(fence=FENCE)), ('fence_keep_out', sub(fence=FENCE, keep_out=[KEEP])),
                ('fence_field', sub(fence=FENCE, wind=fld)), ('t1_window', sub(t1_window=(3.0, 7.0), cost=dur)),
                ('t1_window_keep_out', sub(t1_window=(3.0, 7.0), keep_out=[KEEP], cost=dur)),
                ('t1_window_fence', sub(t1_window=(3.0, 7.0), fence=FENCE, cost=dur)),
                ('t1_window_both', sub(t1_window=(3.0, 7.0), keep_out=[KEEP], fence=FENCE, cost=dur))]
    return [('plain', sub()),
            ('phi_asymmetric', sub(phi_constraint=(-np.deg2rad(25.), np.deg2rad(40.)))),
            ('field', sub(wind=fld)),
            ('moving_disc', sub(moving_obstacles=[_disc(4.)])),
            ('waypoint', sub(waypoints=[d2ou.Waypoint(2.0, 22.0, 5.0)])),
            ('waypoint_disc_field', sub(waypoints=[d2ou.Waypoint(3.5, psi=0.05)], moving_obstacles=[_disc(4.)], wind=fld, t0=2.0, t1=6.0)),
            ('t1_free', sub(t1_free=(3.0, 7.0), cost=d2ou.CostComposit(None, vsp=12., kvel=5., kbank=1., kdur=0.3)))]


def _multi_scenarios(which='parent'):
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
    if which == 'abi129':                        # (keep_out, a MovingKeepOut and t1_window are refused by this planner before any lowering)
        return [('one_fence', sub(p0s=two.p0s[:1], p1s=two.p1s[:1], cost=comp(nan), fence=FENCE)), ('two_fence', sub(fence=FENCE)),
                ('two_uncoupled_fence', sub(cost=comp(nan), fence=FENCE)),
                ('three_pairs_fence', sub(p0s=p3, p1s=q3, cost=comp(10., col_pairs=[(0, 2), (1, 2)]), fence=FENCE))]
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


def _plan_batch_cases(which='parent'):
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
    if which == 'abi129':
        karr = np.array([[[18.0, 70.0, 5.0], [0.0, 0.0, -1.0]]] * 3) + np.arange(3.0)[:, None, None]
        frow = FENCE.lowered()
        hard, hards = [_hard(3.), KEEP], [[_hard(3.)], [_hard(4.)]]
        box = np.array([[0.25, 1.0], [0.3, 0.9], [0.4, 0.8]])
        dec = dict(d_sep=8.0, margin=1.0, d_look=60.0, n_mov=2)
        cases = [('keep_array', solo, 1, dict(keep_out=karr)), ('keep_list', solo, 1, dict(keep_out=[KEEP], opt_tol=1e-6)),
                 ('keep_array_wind', solo, 1, dict(keep_out=karr, windfield=fld, t_start=1.5)),
                 ('keep_list_wind', solo, 1, dict(keep_out=[KEEP, KEEP], windfield=fld, t_start=torch.tensor([0.0, 1.0, 2.5], dtype=torch.float64))),
                 ('fence_solo', solo, 1, dict(fence=FENCE)), ('fence_solo_rows', solo, 1, dict(fence=np.stack([frow] * 3), opt_tol=1e-6)),
                 ('fence_solo_list', solo, 1, dict(fence=[FENCE] * 3)), ('fence_solo_keep', solo, 1, dict(fence=FENCE, keep_out=[KEEP])),
                 ('fence_solo_keep_array', solo, 1, dict(fence=np.stack([frow] * 3), keep_out=karr)),
                 ('fence_solo_wind', solo, 1, dict(fence=FENCE, windfield=fld, t_start=1.5)),
                 ('fence_solo_keep_wind', solo, 1, dict(fence=FENCE, keep_out=karr, windfield=fld, t_start=0.5)),
                 ('fence_masked', masked, 2, dict(fence=FENCE)), ('fence_bare', bare, 2, dict(fence=np.stack([frow] * 2), **kw)),
                 ('fence_half', half, 2, dict(fence=[FENCE, FENCE])), ('fence_pairs', trio, 3, dict(fence=FENCE)),
                 ('fence_bare_wind', bare, 2, dict(fence=FENCE, windfield=fld, t_start=ts, **kw)),
                 ('hard_solo', solo, 1, dict(hard_moving=hard, t_start=1.0)), ('hard_solo_per', solo, 1, dict(hard_moving=[[_hard(3.)]] * 3)),
                 ('hard_bare', bare, 2, dict(hard_moving=hards, t_start=ts)), ('hard_masked', masked, 2, dict(hard_moving=hard, **kw)),
                 ('hard_half', half, 2, dict(hard_moving=hard)), ('hard_pairs', trio, 3, dict(hard_moving=hard, t_start=0.5)),
                 ('hard_solo_wind', solo, 1, dict(hard_moving=hard, windfield=fld, t_start=1.5)),
                 ('hard_bare_wind', bare, 2, dict(hard_moving=hards, windfield=fld, t_start=ts, **kw)),
                 ('window_scalar', solo, 1, dict(window=(0.25, 1.0), kdur=0.4)), ('window_rows', solo, 1, dict(window=box, kdur=np.array([0.0, 0.2, 0.4]))),
                 ('window_keep', solo, 1, dict(window=box, keep_out=[KEEP], kdur=0.4, opt_tol=1e-6)),
                 ('window_keep_array', solo, 1, dict(window=(0.25, 1.0), keep_out=karr)),
                 ('window_fence', solo, 1, dict(window=(0.25, 1.0), fence=FENCE, kdur=0.4)),
                 ('window_both', solo, 1, dict(window=box, keep_out=[KEEP], fence=np.stack([frow] * 3), kdur=np.array([0.0, 0.2, 0.4]))),
                 ('deconflict', bare, 2, dict(deconflict=dec, t_start=ts, **kw)), ('deconflict_masked_wind', masked, 2, dict(deconflict=dec, windfield=fld, t_start=1.5)),
                 ('deconflict_pairs', trio, 3, dict(deconflict=dict(dec, hard=True))), ('deconflict_solo', solo, 1, dict(deconflict=dec)),
                 ('dubins', bare, 2, dict(W0='dubins')), ('dubins_keep', solo, 1, dict(W0='dubins', keep_out=karr)),
                 ('dubins_fence_solo', solo, 1, dict(W0='dubins', fence=FENCE, keep_out=[KEEP])), ('dubins_fence_bare', bare, 2, dict(W0='dubins', fence=FENCE)),
                 ('dubins_hard', bare, 2, dict(W0='dubins', hard_moving=hard)), ('dubins_window', solo, 1, dict(W0='dubins', window=(0.25, 1.0), fence=FENCE)),
                 ('dubins_free', solo, 1, dict(W0='dubins', free_time=(0.25, 1.0))), ('dubins_moving', bare, 2, dict(W0='dubins', moving=disc))]
        return N, h, guess, cases
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


def _deconflict_recorder(calls):
    """Stands where full_sim.deconflict_plans is (the real one needs a device): records its arguments beside the entries' calls."""
    def deconflict_plans(ctx, scen, W, h, n_ac, **kw):
        calls().append({'entry': 'deconflict_plans', 'args': {k: _rec(v) for k, v in dict(scen=scen, W=W, h=h, n_ac=n_ac, **kw).items()}})
        return W, {'recorded': True}
    return deconflict_plans


def collect(which='parent'):
    """{configuration: {'calls': [...], ...}} of every configuration of the set `which` ('parent': nlp_dispatch_parent.json; 'abi129':
    nlp_dispatch_abi129.json), with the recording stand-in as the default context."""
    import full_sim as fs
    import multi_opt_planner as mop
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    real = d2dhip.default_context
    real_plan, real_dec = sop.get_plan, fs.deconflict_plans
    ctx = RecordingContext()
    d2dhip.default_context = lambda: ctx
    fs.deconflict_plans = _deconflict_recorder(lambda: ctx.calls)
    out = {}

    def take(name, **extra):
        out[name] = dict(calls=ctx.calls, **extra)
        ctx.calls = []

    try:
        for name, exp in _single_scenarios(which):
            p = sop.Planner(exp, backend='nlp')
            p.configure(tol=1e-6, max_iter=900)
            p.run()
            take('single/' + name, info=sorted(p.info), backend_used=p.info.get('backend_used'))
        if which == 'parent':
            # a psi box and an asymmetric phi interval, as a caller of opty's Problem spells them
            exp = _single_scenarios()[0][1]
            p = sop.Planner(exp, backend='nlp')
            g = p.aircraft
            bounds = dict(p._bounds)
            bounds[g._spsi(g._st)] = (-1.0, 1.5)
            prob = odc.Problem(p.prob.obj, p.prob.obj_grad, g.get_eom(p.wind), g._state_symbols, p.num_nodes, p.time_step,
                                   known_parameter_map={},
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
        for name, scen in _multi_scenarios(which):
            m = mop.Planner(scen, backend='nlp')
            m.run(tol=1e-6, max_iter=700)
            take('multi/' + name, info=sorted(m.info), backend_used=m.info.get('backend_used'))
        N, h, guess, cases = _plan_batch_cases(which)
        for name, rows, n_ac, kw in cases:
            res = fs.plan_batch(rows.copy(), N, (N - 1) * h, 1.0 / N, backend='nlp', h=h, n_ac=n_ac, **{'W0': guess(rows), **kw})
            take('plan_batch/' + name, scen=_rec(res['scen']), keys=sorted(k for k in res if k != 'entry'))
    finally:
        d2dhip.default_context = real
        sop.get_plan, fs.deconflict_plans = real_plan, real_dec
    return out


PLAN_INPUTS = ('n_ac', 'field', 't_start', 'knots', 'disc', 'via', 'free_rows', 'pairs', 'keep', 'hard_knots', 'hard_disc', 'fence', 'window')
BATCH_FEATURES = ('windfield', 'moving', 'via', 'gust', 'free_time', 'keep_out', 'deconflict', 'hard_moving', 'fence', 'window')


class _Stub:
    """Any object with the nlp_solve* methods: each returns what it was called with."""

    def __getattr__(self, name):
        if not name.startswith('nlp_solve'):
            raise AttributeError(name)
        return lambda *a, **kw: dict(called=name, a=a, kw=kw)


def _outcome(call):
    """call() -> its JSON outcome: what it returns, or the exception's type and full text."""
    try:
        return call()
    except Exception as e:                      # noqa: BLE001  (whatever is raised IS the record)
        return {'raises': type(e).__name__, 'message': str(e)}


def refusals():
    """{'outcomes': the distinct outcomes, 'nlp_plan': [index per subset], 'plan_batch': [index per case]}.  Subsets in the order of
    itertools.product([False, True], repeat=n) over PLAN_INPUTS; plan_batch's cases in the order of product(('fit', 'nlp'), (1, 2),
    subsets of BATCH_FEATURES), then W0='dubins' with via."""
    import full_sim as fs
    import single_opt_planner as sop
    outcomes, index = [], {}

    def idx(o):
        key = json.dumps(o, sort_keys=True)
        if key not in index:
            index[key] = len(outcomes)
            outcomes.append(json.loads(key))
        return index[key]

    values = dict(n_ac=3, pairs=True, **{k: k.upper() for k in PLAN_INPUTS if k not in ('n_ac', 'pairs')})

    def plan(kw):
        out = d2dhip.nlp_plan(_Stub(), 'SCEN', 'W', 0.1, bounds='B', **kw)
        assert out['entry'] == out['called'] and out['a'][:3] == ('SCEN', 'W', 0.1) and out['kw'].pop('bounds') == 'B'
        return {'entry': out['entry'], 'positional': list(out['a'][3:]), 'keywords': dict(sorted(out['kw'].items()))}

    res = {'nlp_plan': [idx(_outcome(lambda: plan({k: values[k] for k, g in zip(PLAN_INPUTS, given) if g})))
                        for given in itertools.product([False, True], repeat=len(PLAN_INPUTS))]}

    N, h, guess, cases = _plan_batch_cases()                 # (replaces sop.get_plan by a stand-in: the fit backend ends at its None)
    rows = {n_ac: next(r for name, r, n, _ in cases if name == want) for n_ac, want in ((1, 'groups_solo'), (2, 'groups_masked'))}
    wp = d2ou.Waypoint(1.5, 20.0, 4.0)
    feats = dict(windfield=_field(), moving=[_disc(3.)], gust=object(), free_time=(0.25, 1.0), keep_out=[KEEP],
                 deconflict=dict(d_sep=8.0, margin=1.0, d_look=60.0), hard_moving=[_hard(3.)], fence=FENCE, window=(0.25, 1.0))
    real, real_plan, real_dec = d2dhip.default_context, sop.get_plan, fs.deconflict_plans
    ctx = RecordingContext()
    d2dhip.default_context = lambda: ctx
    fs.deconflict_plans = _deconflict_recorder(lambda: ctx.calls)

    def batch(backend, n_ac, kw):
        ctx.calls = []
        r = rows[n_ac]
        if 'via' in kw:
            kw = dict(kw, via=[[wp]] + [[]] * (len(r) - 1))
        out = fs.plan_batch(r.copy(), N, (N - 1) * h, 1.0 / N, backend=backend, h=h, n_ac=n_ac, **{'W0': guess(r), **kw})
        return {'entries': [c['entry'] for c in ctx.calls], 'keys': sorted(k for k in out if k != 'entry')}

    try:
        res['plan_batch'] = [idx(_outcome(lambda: batch(backend, n_ac, {k: feats.get(k) for k, g in zip(BATCH_FEATURES, given) if g})))
                             for backend in ('fit', 'nlp') for n_ac in (1, 2)
                             for given in itertools.product([False, True], repeat=len(BATCH_FEATURES))]
        res['plan_batch'].append(idx(_outcome(lambda: batch('nlp', 1, dict(via=True, W0='dubins')))))
    finally:
        d2dhip.default_context = real
        sop.get_plan, fs.deconflict_plans = real_plan, real_dec
    res['outcomes'] = outcomes
    return res


def write_refusals(res, path):
    """One outcome per line and each index on one line: the file stays readable and small."""
    with open(path, 'w') as f:
        f.write('{"outcomes": [\n' + ',\n'.join(' ' + json.dumps(o, sort_keys=True) for o in res['outcomes']) + '\n],\n')
        f.write(',\n'.join(f'"{k}": ' + json.dumps(res[k], separators=(',', ':')) for k in ('nlp_plan', 'plan_batch')) + '}\n')


if __name__ == '__main__':
    which = sys.argv[1] if len(sys.argv) > 1 else 'parent'
    if which == 'refusals':
        res = refusals()
        write_refusals(res, os.path.join(GOLD, 'nlp_dispatch_refusals.json'))
        print(f'{len(res["outcomes"])} distinct outcomes of {len(res["nlp_plan"])} nlp_plan and {len(res["plan_batch"])} plan_batch calls')
    else:
        res = collect(which)
        path = os.path.join(GOLD, f'nlp_dispatch_{which}.json')
        with open(path, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')
        print(f'{path}: {len(res)} configurations, {sum(len(v["calls"]) for v in res.values())} calls')
