"""Timed waypoints of the collocation planner without a GPU: the host side (d2d.opty_utils.Waypoint, its lowering to the table of
d2d_via_points, the Problem's interior instance constraints, the planners' routing and refusals), the ABI (struct, constants, entries)
and the CPU statement tests/nlp_via_ref.py on its catalogue."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nlp_via_ref as V
import nlp_wind_ref as R
import d2d.opty_utils as d2ou
from d2d.opty_utils import Waypoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_waypoint_and_its_lowering():
    import d2dhip
    w = Waypoint(3.0, x=36.0, y=8.0)
    assert (w.mask, Waypoint(1.0, psi=0.2).mask, Waypoint(1.0, y=0.0).mask, Waypoint(1.0, 1.0, 2.0, 3.0).mask) == (3, 4, 2, 7)
    with pytest.raises(ValueError, match='at least one'):
        Waypoint(1.0)
    with pytest.raises(ValueError, match='finite'):
        Waypoint(1.0, x=np.nan)
    # on a node, also with a start time that is no multiple of the step and a time that carries rounding
    tab = d2ou.lower_waypoints([w, Waypoint(0.1 * 3 + 2.5, psi=-0.1)], 0.0 + 0.0, 0.1, 61)
    assert tab.shape == (2, 5) and tab[0].tolist() == [30.0, 3.0, 36.0, 8.0, 0.0]
    assert d2ou.lower_waypoints([Waypoint(2.5 + 0.1 * 7, y=1.0)], 2.5, 0.1, 61)[0].tolist() == [7.0, 2.0, 0.0, 1.0, 0.0]
    # off a node: refused, naming the two nearest node times
    with pytest.raises(ValueError, match=r'not a node time: the nearest nodes are at 3\.0\d* and 3\.1'):
        d2ou.lower_waypoints([Waypoint(3.04, x=1.0)], 0.0, 0.1, 61)
    # the first and the last node carry the end conditions
    for t in (0.0, 6.0):
        with pytest.raises(ValueError, match='end conditions'):
            d2ou.lower_waypoints([Waypoint(t, x=1.0)], 0.0, 0.1, 61)
    with pytest.raises(ValueError, match='outside the plan'):
        d2ou.lower_waypoints([Waypoint(7.0, x=1.0)], 0.0, 0.1, 61)
    with pytest.raises(ValueError, match='same component'):
        d2ou.lower_waypoints([Waypoint(3.0, x=1.0), Waypoint(3.0, x=1.0, y=2.0)], 0.0, 0.1, 61)
    assert d2ou.lower_waypoints([Waypoint(3.0, x=1.0), Waypoint(3.0, y=2.0)], 0.0, 0.1, 61)[:, :2].tolist() == [[30, 1], [30, 2]]
    # ragged lists fit one table shape: padded with rows of mask 0
    pad = d2ou.lower_waypoints([w], 0.0, 0.1, 61, 4)
    assert pad.shape == (4, 5) and (pad[1:] == 0.0).all() and pad[0, 1] == 3.0
    assert d2ou.lower_waypoints([], 0.0, 0.1, 61, 2).tolist() == [[0.0] * 5] * 2
    many = [Waypoint(0.1 * k, x=float(k)) for k in range(1, d2dhip.MAX_VIA + 2)]
    with pytest.raises(ValueError, match=f'at most {d2dhip.MAX_VIA} waypoints'):
        d2ou.lower_waypoints(many, 0.0, 0.1, 61)
    assert d2ou.lower_waypoints(many[:-1], 0.0, 0.1, 61).shape == (d2dhip.MAX_VIA, 5)


def test_via_guess_goes_through_the_waypoints():
    x, y, psi, phi, v = d2ou.via_guess((0, 0, 0), (72, 0, 0), [Waypoint(4.0, 48.0, -3.0), Waypoint(2.0, 24.0, 3.0), Waypoint(3.0, psi=0.1)],
                                       0.0, 0.1, 61, 12.0)
    assert (x[20], y[20], x[40], y[40]) == (24.0, 3.0, 48.0, -3.0) and (x[0], y[0], x[60], y[60]) == (0.0, 0.0, 72.0, 0.0)
    assert abs(psi[5] - np.arctan2(3.0, 24.0)) <= 1e-15 and abs(psi[30] - np.arctan2(-6.0, 24.0)) <= 1e-15 and psi[50] > 0
    assert (phi == 0).all() and (v == 12.0).all()
    assert np.allclose(np.diff(x[:21]), 1.2) and np.allclose(np.diff(y[20:41]), -0.3)


def test_abi_struct_constants_and_entries():
    import d2dhip
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_MAX_VIA (\d+)', hdr).group(1)) == d2dhip.MAX_VIA == 16
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 116
    S = d2dhip.ViaPointsC
    assert C.sizeof(S) == 16 and [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [('n_via', 0), ('pts', 8)]
    body = re.search(r'typedef struct \{([^}]*)\} d2d_via_points;', hdr).group(1)
    assert re.findall(r'(\w+);\s+/\*', body) == [f[0] for f in S._fields_]
    for name in ('d2d_nlp_solve_via', 'd2d_nlp_solve_groups_via'):
        assert name in d2dhip.EXPORTS and re.search(r'\bint ' + name + r'\(', hdr)
    assert hasattr(d2dhip.Context, 'nlp_solve_via') and hasattr(d2dhip.Context, 'nlp_solve_groups_via')


def _exp(**kw):
    import single_opt_planner as sop

    class exp(sop.exp_1):
        p0 = (0., 0., 0., 0., 12.)
        t1, p1 = 6., (72., 0., 0., 0., 12.)
    for k, v in kw.items():
        setattr(exp, k, v)
    return exp


def test_problem_takes_a_third_instance_time():
    """Problem(instance_constraints=...) with interior times builds and exposes the pins; the ends stay the end conditions."""
    import single_opt_planner as sop
    p = sop.Planner(_exp(waypoints=[Waypoint(3.0, 36.0, 8.0), Waypoint(4.5, psi=0.0)]), backend='nlp')
    pr = p.prob
    assert pr.t_start == 0.0 and pr.p0s.tolist() == [[0.0, 0.0, 0.0]] and pr.p1s.tolist() == [[72.0, 0.0, 0.0]]
    assert [(w.t, w.mask) for w in pr.waypoints[0]] == [(3.0, 3), (4.5, 4)]
    assert pr.via.shape == (1, 2, 5) and pr.via[0].tolist() == [[30.0, 3.0, 36.0, 8.0, 0.0], [45.0, 4.0, 0.0, 0.0, 0.0]]
    assert pr.objective == 'lowered'
    # directly, as the reference's call does
    import opty.direct_collocation as odc
    g = p.aircraft
    cons = p._instance_constraints + (g._sy(1.0) - 2.0,)
    pr2 = odc.Problem(pr.obj, pr.obj_grad, g.get_eom(p.wind), g._state_symbols, p.num_nodes, p.time_step, known_parameter_map={},
                      instance_constraints=cons, bounds=p._bounds, cost=p.exp.cost, planner=p)
    assert pr2.via[0][:, :2].tolist() == [[10.0, 2.0], [30.0, 3.0], [45.0, 4.0]]
    with pytest.raises(ValueError, match='not a node time'):
        odc.Problem(pr.obj, pr.obj_grad, g.get_eom(p.wind), g._state_symbols, p.num_nodes, p.time_step, known_parameter_map={},
                    instance_constraints=p._instance_constraints + (g._sy(1.03) - 2.0,), bounds=p._bounds, cost=p.exp.cost, planner=p)
    # without interior times nothing changes
    q = sop.Planner(_exp(), backend='nlp')
    assert q.prob.via is None and q.prob.waypoints == [[]] and q.waypoints == []


def test_planner_routing_and_refusals():
    import d2dhip
    import single_opt_planner as sop
    import multi_opt_planner as mop
    import full_sim as fs
    wp = [Waypoint(3.0, 36.0, 8.0)]
    with pytest.raises(NotImplementedError, match="backend='fit' cannot plan through timed waypoints"):
        sop.Planner(_exp(waypoints=wp), backend='fit')
    # 'auto' goes to the collocation problem
    import opty.direct_collocation as odc
    p = sop.Planner(_exp(waypoints=wp))
    assert p.backend == 'auto' and isinstance(p.prob, odc.Problem) and p.prob.via is not None
    g = p.get_initial_guess('via')
    assert g[p._slice_x][30] == 36.0 and g[p._slice_y][30] == 8.0 and (g[p._slice_v] == 12.0).all()
    # the guesses of a scenario without waypoints do not change
    q = sop.Planner(_exp())
    assert not isinstance(q.prob, odc.Problem) and np.array_equal(q.get_initial_guess('tri'), sop.Planner(_exp(waypoints=None)).get_initial_guess('tri'))

    class UserCost:
        def cost(self, free, planner): return float(np.sum(free ** 2))
        def cost_grad(self, free, planner): return 2.0 * free
    with pytest.raises(NotImplementedError, match='timed waypoints together with a host objective'):
        sop.Planner(_exp(waypoints=wp, cost=UserCost()))
    with pytest.raises(ValueError, match='list of d2d.opty_utils.Waypoint'):
        sop.Planner(_exp(waypoints=[(3.0, 36.0, 8.0)]))

    class multi(mop.trap_4):
        p0s = ((0., 0., 0., 0., 12.), (0., 20., 0., 0., 12.)); p1s = ((60., 0., 0., 0., 12.), (60., 20., 0., 0., 12.)); t1 = 5.
        waypoints = [[Waypoint(2.5, 30.0, 3.0)], []]
    with pytest.raises(NotImplementedError, match="backend='fit' cannot plan through timed waypoints"):
        mop.Planner(multi, backend='fit')
    m = mop.Planner(multi)
    assert isinstance(m.prob, odc.Problem) and m.prob.via.shape == (2, 1, 5)
    assert m.prob.via[0].tolist() == [[25.0, 3.0, 30.0, 3.0, 0.0]] and (m.prob.via[1] == 0.0).all()
    gm = m.get_initial_guess('via')
    assert gm[m._slice_x[0]][25] == 30.0 and gm[m._slice_y[0]][25] == 3.0 and gm[m._slice_y[1]][25] == 20.0

    class wrong(multi):
        waypoints = [Waypoint(2.5, 30.0, 3.0)]
    with pytest.raises(ValueError, match='per aircraft'):
        mop.Planner(wrong)
    with pytest.raises(NotImplementedError, match='timed waypoints'):
        fs.plan_batch(np.zeros((1, d2dhip.SCEN_STRIDE)), 61, 6.0, 1.0 / 61, backend='fit', via=[wp])


def _cases():
    return [('const', n) for n in V.catalogue('const')] + [('gust', n) for n in V.catalogue('gust')]


@pytest.mark.parametrize('wind, name', _cases())
def test_the_catalogue_converges_and_its_status_is_stable(wind, name):
    """Every catalogue case: CONVERGED with feas <= 1e-8 from guess(), the recorded cost, the pins held exactly, and the same status
    under a 1e-9 perturbation of the guess (the rule of tests/test_moving_obstacles_cpu.py)."""
    F, t0 = (None, 0.0) if wind == 'const' else (R.fields()['gust'], V.GUST_T_START)
    r, tab = V.catalogue(wind)[name]
    W0 = V.guess(r, tab)
    W, info = V.solve(V.problem(r, tab), W0, F, t0)
    Wp, ip = V.solve(V.problem(r, tab), W0 + 1e-9 * np.random.default_rng(1).standard_normal(W0.shape), F, t0)
    print(f'{name}: cost {info["cost"]:.6f}, feas {info["feas"]:.1e}, steps {info["inner"]} / {ip["inner"]}, perturbed plan moved {np.abs(W - Wp).max():.1e}')
    assert info['status'] == ip['status'] == 1 and info['feas'] <= 1e-8 and ip['feas'] <= 1e-8
    assert abs(info['cost'] - V.COSTS[name]) <= 5e-6 and np.abs(W - Wp).max() <= 1e-5 and info['inner'] == V.STEPS[name]
    assert d2ou.waypoint_error(tab, W.T) == 0.0


def test_the_unreachable_point_stalls():
    r, _ = V.catalogue()['point']
    W0 = V.guess(r, V.UNREACHABLE)
    W, info = V.solve(V.problem(r, V.UNREACHABLE), W0)
    Wp, ip = V.solve(V.problem(r, V.UNREACHABLE), W0 + 1e-9 * np.random.default_rng(1).standard_normal(W0.shape))
    assert info['status'] == ip['status'] == 4 and abs(info['feas'] - 5.844) <= 1e-3 and info['inner'] == 41


@pytest.mark.parametrize('name', list(V.shapes()))
def test_the_shapes_converge(name):
    """The other node counts: CONVERGED, stable under the perturbation, and the step count and cost nlp_via_ref's docstring lists."""
    N, r, tab = V.shapes()[name]
    W0 = V.guess(r, tab, N)
    W, info = V.solve(V.problem(r, tab, N), W0)
    Wp, ip = V.solve(V.problem(r, tab, N), W0 + 1e-9 * np.random.default_rng(1).standard_normal(W0.shape))
    assert info['status'] == ip['status'] == 1 and info['feas'] <= 1e-8 and np.abs(W - Wp).max() <= 1e-5
    steps, cost = V.SHAPES_MEASURED[name]
    assert info['inner'] == steps and abs(info['cost'] - cost) <= 5e-6 and d2ou.waypoint_error(tab, W.T) == 0.0
