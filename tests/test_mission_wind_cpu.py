"""CPU checks of the mission in a wind field: the block Gauss-Seidel statement tests/nlp_groups_wind_ref.py against oracle/nlp.py in a
uniform field, the scenarios it chose for tests/test_gpu_mission_wind.py, and the host side of full_sim (signatures, refusals) up to
the first device call."""
import inspect

import numpy as np
import pytest

import nlp_groups_wind_ref as G
import nlp_wind_ref as R
from oracle import nlp


def test_statement_in_a_uniform_field_equals_the_oracle_alternation():
    """The statement in uniform_field(c) against the same alternation over oracle.nlp.solve with the constant wind c in the Problems:
    same sweep count, every aircraft's cost within 1e-7 relative, nodes within 1e-5."""
    c = (1.0, -0.5)
    rows = G.group_scenarios()[1]
    pbs_f = G.problems_of(rows)
    Wf, inf_f, sw_f, mv_f = G.solve_groups(pbs_f, G.guesses(rows), G.in_field(R.uniform_field(c), 3.0))
    pbs_c = G.problems_of(rows)
    for pb in pbs_c:
        pb.wind = c
    Wc, inf_c, sw_c, mv_c = G.solve_groups(pbs_c, G.guesses(rows), G.in_constant_wind())
    print(f'sweeps {sw_f} / {sw_c}, moved {mv_f:.2e} / {mv_c:.2e}')
    assert sw_f == sw_c and 1 <= sw_f <= 12 and mv_f <= 1e-7 and mv_c <= 1e-7
    for a in range(G.N_AC):
        print(f'  aircraft {a}: cost {inf_f[a]["cost"]:.12f} / {inf_c[a]["cost"]:.12f}, nodes {np.abs(Wf[a] - Wc[a]).max():.2e}')
        assert inf_f[a]['status'] == 1 and inf_c[a]['status'] == 1
        assert abs(inf_f[a]['cost'] - inf_c[a]['cost']) <= 1e-7 * max(inf_c[a]['cost'], 1e-3)
        assert np.abs(Wf[a] - Wc[a]).max() <= 1e-5
        assert np.abs(nlp.constraints(pbs_c[a], Wf[a])).max() <= 1e-8


@pytest.mark.parametrize('name', ['shear', 'vortex', 'gust'])
def test_the_chosen_scenarios_are_what_their_docstring_says(name):
    """What group_scenarios' docstring claims, asserted for every scenario in every field: the UNCOUPLED solutions of aircraft 0 and 1
    come within rcol of each other (the partner's term is exercised); every inner solve converges and the pair settles within the 12
    sweeps that are Problem's default at sweep_tol 1e-7; under a 1e-9 perturbation of the guess the sweep count does not change and
    no aircraft's Newton-step count moves by more than 10 (the bar the single-aircraft tests hold step counts to)."""
    F = R.fields()[name]
    rng = np.random.default_rng(1)
    for k, rows in enumerate(G.group_scenarios()):
        t0 = G.T_STARTS[name][k]
        pbs = G.problems_of(rows)
        W0 = G.guesses(rows)
        Wu = [R.solve(R.FieldProblem(pbs[a], F, t0), W0[a]) for a in (0, 1)]
        assert Wu[0][1]['status'] == 1 and Wu[1][1]['status'] == 1
        d = float(np.hypot(Wu[0][0][:, 0] - Wu[1][0][:, 0], Wu[0][0][:, 1] - Wu[1][0][:, 1]).min())
        assert pbs[0].kcol > 0.0 and pbs[0].rcol == G.RCOL and d < G.RCOL
        Ws, infos, sweeps, moved = G.solve_groups(pbs, W0, G.in_field(F, t0))
        Wp, infos_p, sweeps_p, moved_p = G.solve_groups(G.problems_of(rows), [w + 1e-9 * rng.standard_normal(w.shape) for w in W0], G.in_field(F, t0))
        steps, steps_p = [i['inner'] for i in infos], [i['inner'] for i in infos_p]
        print(f'{name} scenario {k}: the uncoupled plans come within {d:.2f} m (rcol {G.RCOL}); sweeps {sweeps} / {sweeps_p}, moved {moved:.1e}, '
              f'Newton steps {steps} / {steps_p} under the perturbation')
        assert all(i['status'] == 1 for i in infos) and 1 <= sweeps <= 12 and moved <= 1e-7, (sweeps, moved)
        assert sweeps_p == sweeps and max(abs(a - b) for a, b in zip(steps, steps_p)) <= 10
        assert np.abs(Ws[0][:, :2] - Wu[0][0][:, :2]).max() > 1e-6           # the coupling moved the pair


def test_the_mission_field_is_unsteady_where_the_mission_flies():
    """mission_field: the constant (1, 0) before 100 s, then growing; two times one phase-1 row apart see winds that differ by what
    mission_wind's docstring says, and the spline is the function (it is linear in t)."""
    F = G.mission_field()
    x = np.linspace(-60.0, 120.0, 19); y = np.linspace(-150.0, 40.0, 19)
    wx0, wy0 = F.sample_many(50.0, x, y)
    assert np.abs(wx0 - 1.0).max() <= 1e-12 and np.abs(wy0).max() <= 1e-12
    a, b = F.sample_many(134.0, x, y), F.sample_many(134.05, x, y)
    assert np.abs(b[0] - a[0]).min() >= 2.5e-4 * (1 - 1e-9)
    fx, fy = G.mission_wind(134.0, x, y)
    assert np.abs(a[0] - fx).max() <= 1e-12 and np.abs(a[1] - fy).max() <= 1e-12


def test_signatures_and_refusals_before_the_first_device_call():
    """plan_batch and full_sim_phases_batch take the field as keywords that default to today's path, and refuse a foreign field
    object before they touch the device."""
    import full_sim as fs
    import multi_opt_planner as mop
    sig = inspect.signature(fs.full_sim_phases_batch)
    assert sig.parameters['windfield'].default is None
    sig = inspect.signature(fs.plan_batch)
    assert sig.parameters['windfield'].default is None and sig.parameters['t_start'].default == 0.0

    class Foreign:
        def sample(self, t, loc):
            return np.array([np.sin(t), 0.0])

        def sample_sym(self, t, x, y):
            return (x, y)

    c = np.zeros((1, 4, 2)); X = np.zeros((4, 5))
    with pytest.raises(NotImplementedError, match='SplineWindField.from_field'):
        fs.full_sim_phases_batch(c, 60, 15, 4, X, mop.trap_4, X, 6, windfield=Foreign())
    with pytest.raises(NotImplementedError, match='SplineWindField.from_field'):
        fs.plan_batch(np.zeros((4, 1)), 61, None, None, backend='nlp', W0=np.zeros((4, 5, 61)), h=0.1, n_ac=4, windfield=Foreign())
    with pytest.raises(NotImplementedError, match='polynomial fit has no wind field'):
        fs.plan_batch(np.zeros((4, 1)), 61, 6.0, 1.0, windfield=R.uniform_field((1.0, 0.0)))


def test_binding_declares_the_new_entry_points():
    import d2dhip
    assert 'd2d_nlp_solve_groups_wind' in d2dhip.EXPORTS and 'd2d_sim_track_run_wind_at' in d2dhip.EXPORTS
    assert hasattr(d2dhip.Context, 'nlp_solve_groups_wind')
