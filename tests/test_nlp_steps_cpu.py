"""CPU: the cases of the Newton-step-by-Newton-step comparison (tests/nlp_steps_ref.py, tests/test_gpu_nlp_steps.py) are fit for it, by
the CPU statements alone -- so that the GPU test cannot hide a failure behind a case that says nothing:

  determined          after every budget the tolerance measured on the statement (8 starts moved by an ulp, margin 1e3) is <= 1e-8
                      and the perturbed runs take the unperturbed run's path: the same step counts, raises of the damping, halvings
                      and step lengths;
  not finished early  after every budget with outer_max = 1 the statement reports 'max iterations', every counted step was accepted
                      (none of them the convergence test) and each moved W by more than 1e6 tol.

A case that fails is replaced by another input (the seed tables of tests/nlp_steps_ref.py), never skipped or given a wider margin.
The statement of d2d_nlp_solve_model (tests/nlp_model_ref.py) is checked here against the oracle and against finite differences.

Floors measured on this run (largest |dW| of the statement's iterate over the 8 perturbed starts, over the budgets):
  d2d_nlp_solve         3, 5 nodes 2e-17 .. 2e-13;  64 .. 129 nodes 3e-14 .. 8e-12;  with bounds (41 nodes) 5e-15 .. 3e-12
  d2d_nlp_solve_wind    41 nodes 7e-15 .. 1e-12;  65 nodes 1e-14 .. 5e-12;  122 nodes 3e-14 .. 9e-12
  d2d_nlp_solve_moving  constant wind 2e-14 .. 6e-13;  gust 7e-15 .. 1e-11
  d2d_nlp_solve_model   5 nodes 2e-16 .. 4e-14;  41, 65 nodes 4e-15 .. 8e-12
  d2d_nlp_solve_groups* (41 nodes, 2 and 3 aircraft, 1 and 2 sweeps)  5e-15 .. 9e-12 in every one of the five entries
"""
import numpy as np
import pytest

import nlp_model_ref as MR
import nlp_steps_ref as S
from oracle import nlp


@pytest.mark.parametrize('lid', S.launch_ids())
def test_cases_are_determined_and_not_finished_early(lid):
    L = S.launch(lid)
    bad = []
    for case in L.cases:
        for budget in S.BUDGETS:
            m = S.measure(case, budget)
            print(f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {m["tol"]:.1e}, steps {m["info"]["inner"]}')
            bad += [(case.cid, budget, c) for c in S.check(case, budget)]
    assert not bad, bad


def test_every_listed_shape_has_a_launch():
    ids = S.launch_ids()
    assert len(set(ids)) == len(ids)
    assert [S.launch(f'plain-{N}').N for N in (3, 5, 64, 65, 121, 122, 129)] == [3, 5, 64, 65, 121, 122, 129]
    assert all(len(S.launch(f'plain-{N}').cases) == 4 for N in S.PLAIN_N)
    assert all(f'wind-{f}-{N}' in ids for f in ('shear', 'vortex', 'gust') for N in (41, 65, 122))
    assert all(L.N <= 130 and len(L.cases) * L.kw.get('n_ac', 1) <= 8 for L in map(S.launch, ids))
    for e in S.GROUP_ENTRIES:
        for sw in (1, 2):
            names = {c.cid.split('-')[-1] for lid in ids if lid.startswith(f'{e}-3-sweeps{sw}') for c in S.launch(lid).cases}
            assert names == ({'pair'} if e in ('groups', 'groupswind') else {'pair', 'chain', 'all'})
            assert f'{e}-2-sweeps{sw}' in ids
    ts = S.launch('moving-gust').kw['t_start']
    assert len(set(ts)) == 2                                     # two start times in one launch
    assert S.BUDGETS == ((1, 1), (2, 1), (3, 1), (5, 1), (8, 1), (5, 2), (5, 3), (5, 4))


def test_plane_order_is_the_header_s():
    """include/d2d.h: plane a*5 - a*(a-1)/2 + (c-a) holds H[a][c], a <= c."""
    H = np.arange(25.0).reshape(1, 5, 5); H = H + H.transpose(0, 2, 1)
    planes = MR.pack(H)
    for a in range(5):
        for c in range(a, 5):
            assert planes[a * 5 - a * (a - 1) // 2 + (c - a), 0] == H[0, a, c]
    np.testing.assert_array_equal(MR.unpack(planes), H)


def test_model_statement_with_an_empty_model_is_the_oracle():
    """nlp_wind_ref.solve through a ModelProblem whose model is zero = oracle.nlp.solve on the same Problem, bit for bit: the loop the
    model statement borrows is the oracle's."""
    mp, _, W0 = S.model_problem(41, 'spd', 3)
    zero = MR.ModelProblem(mp.pb, 0.0 * mp.g, 0.0 * mp.H, mp.Wc)
    for budget in ((8, 1), (5, 4)):
        Wm, im = MR.solve(zero, W0, inner_max=budget[0], outer_max=budget[1])
        Wo, io = nlp.solve(mp.pb, W0, inner_max=budget[0], outer_max=budget[1])
        assert np.array_equal(Wm, Wo) and im['inner'] == io['inner'] and im['path'] == io['path'] and np.array_equal(im['mult'], io['mult'])


@pytest.mark.parametrize('kind', ['spd', 'partial', 'indefinite'])
def test_model_statement_against_finite_differences(kind):
    """The statement's half gradient is half the gradient of its own merit function (central differences, every free entry of a
    5-node problem), and its diagonal blocks gain exactly H / 2."""
    mp, _, W0 = S.model_problem(5, kind, 11)
    pb = mp.pb
    fixed, hasL, hasU = nlp._barrier_sets(pb)
    W = np.clip(W0, pb.lo + 0.05, pb.hi - 0.05); W[fixed] = pb.lo[fixed]
    mu = 0.01 * np.arange(12.0).reshape(4, 3); rho = 10.0
    g, D, E = mp.normal_equations(W, mu, rho)
    g0, D0, E0 = nlp._normal_equations(pb, W, mu, rho)
    np.testing.assert_allclose(D - D0, 0.5 * mp.H, rtol=0, atol=1e-10)          # (D0 holds rho / h^2 = 1e3: the difference rounds at 1e-13)
    assert np.array_equal(E, E0)
    none = np.zeros_like(hasL)
    for i, c in zip(*np.nonzero(~fixed)):
        e = np.zeros_like(W); e[i, c] = 1e-6
        fd = (mp.merit(W + e, mu, rho, 0.0, none, none) - mp.merit(W - e, mu, rho, 0.0, none, none)) / 2e-6
        assert abs(fd - 2.0 * g[i, c]) <= 1e-6 * max(1.0, abs(fd)), (i, c, fd, 2.0 * g[i, c])
    d = W - mp.Wc
    assert mp.value(W) == pytest.approx(sum(mp.g[i] @ d[i] + 0.5 * d[i] @ mp.H[i] @ d[i] for i in range(5)), rel=1e-14)


def test_indefinite_model_raises_the_damping():
    """The indefinite model makes the statement raise its damping eightfold (a failed factorisation or an ascent direction) within
    the first eight steps -- the retry the GPU comparison is to follow."""
    case = S.launch('model-indefinite-41').cases[0]
    path = S.measure(case, (8, 1))['info']['path']
    assert len(path) == 8 and sum(p[2] for p in path) >= 1, path
