"""Moving obstacles of the collocation planner without a GPU: the host side (d2d.opty_utils.MovingObstacle, its lowering to the
tables of d2d_moving_obstacles, the planners' refusals), the ABI (struct size, constants in header = binding) and the CPU statement
tests/nlp_moving_ref.py on its catalogue of starting scenarios."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nlp_moving_ref as M
import nlp_wind_ref as R
import d2d.opty_utils as d2ou
from d2d.opty_utils import MovingObstacle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_at_is_linear_interpolation_held_outside_the_knots():
    rng = np.random.default_rng(0)
    tk = np.cumsum(rng.uniform(0.1, 3.0, 7)) + 20.0
    o = MovingObstacle(tk, rng.uniform(-150, 150, (7, 2)), 4.0)
    t = np.concatenate([[tk[0] - 5.0, tk[0], tk[-1], tk[-1] + 5.0], tk[2:4], rng.uniform(tk[0] - 1, tk[-1] + 1, 200)])
    ref = np.stack([np.interp(t, tk, o.xy[:, 0]), np.interp(t, tk, o.xy[:, 1])], -1)
    np.testing.assert_allclose(o.at(t), ref, rtol=0, atol=1e-12)
    assert np.array_equal(o.at(tk[0] - 5.0), o.xy[0]) and np.array_equal(o.at(tk[-1] + 5.0), o.xy[-1])
    assert np.array_equal(o.at(tk), o.xy)                       # a knot exactly at its time
    # padding repeats the last knot at strictly later times and changes no centre
    p = o.padded(12)
    assert p.shape == (12, 3) and (np.diff(p[:, 0]) > 0).all() and np.array_equal(p[:7, 0], tk) and (p[7:, 1:] == o.xy[-1]).all()
    assert np.array_equal(d2ou.track_at(p[:, 0], p[:, 1:], t), o.at(t))
    lin = MovingObstacle.linear((36.0, -28.0), (0.0, 10.0), 8.0, t0=2.0, t1=12.0)
    np.testing.assert_allclose(lin.at(np.array([0.0, 2.0, 5.0, 12.0, 13.0])), [(36, -28), (36, -28), (36, 2), (36, 72), (36, 72)], atol=1e-12)


def test_lowering_to_the_tables():
    a = MovingObstacle((0.0, 1.0, 4.0), ((0, 0), (1, 1), (2, 0)), 3.0, kind=0)
    b = MovingObstacle.linear((5.0, 5.0), (1.0, 0.0), 2.0, t0=1.0, t1=3.0)
    kn, dc = d2ou.lower_moving([a, b])
    assert kn.shape == (2, 3, 3) and dc.tolist() == [[3.0, 0.0], [2.0, 1.0]]
    assert np.array_equal(kn[0], [(0, 0, 0), (1, 1, 1), (4, 2, 0)]) and np.array_equal(kn[1, :2], [(1, 5, 5), (3, 7, 5)])
    assert kn[1, 2, 0] > 3.0 and np.array_equal(kn[1, 2, 1:], (7, 5))
    kn5, _ = d2ou.lower_moving([a, b], 5)
    assert kn5.shape == (2, 5, 3) and (np.diff(kn5[:, :, 0], axis=1) > 0).all()
    kn0, dc0 = d2ou.lower_moving([])
    assert kn0.shape[0] == 0 and dc0.shape == (0, 2)


def test_refusals():
    import d2dhip
    import single_opt_planner as sop
    import multi_opt_planner as mop
    with pytest.raises(ValueError, match='increase strictly'):
        MovingObstacle((0.0, 1.0, 1.0), ((0, 0), (1, 1), (2, 2)), 1.0)
    with pytest.raises(ValueError, match='finite'):
        MovingObstacle((0.0, 1.0), ((0, np.nan), (1, 1)), 1.0)
    with pytest.raises(ValueError, match='kind'):
        MovingObstacle((0.0, 1.0), ((0, 0), (1, 1)), 1.0, kind=2)
    one = MovingObstacle.linear((0, 0), (1, 0), 2.0)
    with pytest.raises(NotImplementedError, match=f'at most {d2dhip.MAX_MOV} moving obstacles'):
        d2ou.lower_moving([one] * (d2dhip.MAX_MOV + 1))
    n = d2dhip.MOV_MAX_KNOT + 1
    with pytest.raises(ValueError, match=f'at most {d2dhip.MOV_MAX_KNOT} knots'):
        d2ou.lower_moving([MovingObstacle(np.arange(n), np.zeros((n, 2)), 1.0)])

    class exp(sop.exp_1):
        p0 = (0., 0., 0., 0., 12.)
        moving_obstacles = [one]
    with pytest.raises(NotImplementedError, match="backend='fit' cannot plan around moving obstacles"):
        sop.Planner(exp, backend='fit')

    class many(exp):
        moving_obstacles = [one] * (d2dhip.MAX_MOV + 1)
    with pytest.raises(NotImplementedError, match='moving obstacles per problem'):
        sop.Planner(many)

    class UserCost:
        def cost(self, free, planner): return float(np.sum(free ** 2))
        def cost_grad(self, free, planner): return 2.0 * free

    class user(exp):
        cost = UserCost()
    with pytest.raises(NotImplementedError, match='moving obstacles together with a host objective'):
        sop.Planner(user)

    class multi(mop.trap_4):
        p0s = ((0., 0., 0., 0., 12.), (0., 20., 0., 0., 12.)); p1s = ((60., 0., 0., 0., 12.), (60., 20., 0., 0., 12.)); t1 = 5.
        moving_obstacles = [one]
    with pytest.raises(NotImplementedError, match="backend='fit' cannot plan around moving obstacles"):
        mop.Planner(multi, backend='fit')
    # without the attribute, or with an empty list, nothing changes
    assert sop.Planner(sop.exp_0, initialize=False).moving_obstacles == []
    import full_sim as fs
    with pytest.raises(NotImplementedError, match='moving'):
        fs.plan_batch(np.zeros((1, d2dhip.SCEN_STRIDE)), 61, 6.0, 1.0 / 61, backend='fit', moving=[one])


def test_abi_struct_and_constants():
    import d2dhip
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_MAX_MOV (\d+)', hdr).group(1)) == d2dhip.MAX_MOV == 8
    assert int(re.search(r'#define D2D_MOV_MAX_KNOT (\d+)', hdr).group(1)) == d2dhip.MOV_MAX_KNOT == 32
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 115
    S = d2dhip.MovingObstaclesC
    assert C.sizeof(S) == 24 and [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [('n_mov', 0), ('n_knot', 4), ('knots', 8), ('disc', 16)]
    body = re.search(r'typedef struct \{([^}]*)\} d2d_moving_obstacles;', hdr).group(1)
    assert re.findall(r'(\w+);\s+/\*', body) == [f[0] for f in S._fields_]
    for name in ('d2d_mov_sample', 'd2d_nlp_solve_moving', 'd2d_nlp_solve_groups_moving'):
        assert name in d2dhip.EXPORTS and re.search(r'\bint ' + name + r'\(', hdr)


@pytest.mark.parametrize('wind, kind, name, leg, t0', M.cases())
def test_the_catalogue_converges_and_its_status_is_stable(wind, kind, name, leg, t0):
    """Every starting scenario, both kinds, in still air and in the gust: CONVERGED with feas <= 1e-8 from the straight-line guess,
    and the same status under a 1e-9 perturbation of the guess (what the pairs catalogue was held to); the plan goes round the disc."""
    F = None if wind == 'const' else R.fields()['gust']
    mv = M.catalogue(kind, t0, leg)[name]
    r = M.row(kind, p1=(leg, 0.0, 0.0))
    W0 = M.straight_guess(r)
    W, info = M.solve(M.problem(r, mv, t0), W0, F, t0)
    Wp, ip = M.solve(M.problem(r, mv, t0), W0 + 1e-9 * np.random.default_rng(1).standard_normal(W0.shape), F, t0)
    print(f'{wind} kind {kind} {name}: cost {info["cost"]:.4f}, feas {info["feas"]:.1e}, steps {info["inner"]} / {ip["inner"]}, '
          f'detour {np.abs(W[:, 1]).max():.2f} m, perturbed plan moved {np.abs(W - Wp).max():.1e}')
    assert info['status'] == ip['status'] == 1 and info['feas'] <= 1e-8 and ip['feas'] <= 1e-8
    assert np.abs(W[:, 1]).max() > 3.0 and np.abs(W - Wp).max() <= 1e-5
    if wind == 'const':          # the costs the scenarios were chosen with
        ref = {('crossing', 1): 1.3708, ('crossing', 0): 7.8155, ('headon', 1): 0.7802, ('headon', 0): 3.1357, ('two', 1): 1.3838, ('two', 0): 7.8155}
        assert abs(info['cost'] - ref[name, kind]) <= 5e-5


def test_a_disc_that_has_passed_changes_nothing():
    """The statement reads the track at the nodes' own times: the crossing anchored 100 s earlier is long gone and the plan is the straight line."""
    r = M.row(1)
    W, info = M.solve(M.problem(r, M.catalogue(1, -100.0)['crossing'], 0.0), M.straight_guess(r))
    assert info['status'] == 1 and np.abs(W[:, 1]).max() <= 1e-6
