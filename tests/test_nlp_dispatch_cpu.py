"""The planners' choice among the collocation entries (d2dhip.nlp_plan), without a GPU.

1. Same routing as before the ladders were folded: tests/golden/make_nlp_dispatch_golden.py drives Problem.solve (through both
   planners) and plan_batch over a recording stand-in of the context; tests/golden/nlp_dispatch_parent.json is what it recorded at
   the commit before the fold.  Every call -- entry, rows, tables, options -- must be the same.
2. The rule itself: nlp_plan with every combination of the optional inputs lands on the entry its table names, and hands it the
   inputs that entry takes."""
import importlib.util
import itertools
import json
import os

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def maker():
    spec = importlib.util.spec_from_file_location('make_nlp_dispatch_golden', os.path.join(GOLD, 'make_nlp_dispatch_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def replay(maker):
    with open(os.path.join(GOLD, 'nlp_dispatch_parent.json')) as f:
        parent = json.load(f)
    return parent, json.loads(json.dumps(maker.collect()))        # (through JSON: tuples become lists, as in the file)


def test_every_configuration_is_replayed(replay):
    parent, now = replay
    assert sorted(now) == sorted(parent) and len(parent) >= 40
    for need in ('single/plain', 'single/phi_asymmetric', 'single/psi_box', 'single/field', 'single/moving_disc', 'single/waypoint',
                 'single/waypoint_disc_field', 'single/t1_free', 'single/auto_harden', 'multi/one_aircraft', 'multi/two_default_pair',
                 'multi/two_uncoupled', 'multi/three_pairs', 'multi/two_discs', 'multi/two_waypoints', 'multi/two_waypoints_discs',
                 'plan_batch/via_solo', 'plan_batch/groups_masked', 'plan_batch/groups_bare', 'plan_batch/free_scalar', 'plan_batch/free_rows'):
        assert need in parent
    # every entry a stand-in can be sent to is reached (nlp_solve itself and nlp_solve_model are no planner's choice)
    assert {c['entry'] for v in parent.values() for c in v['calls']} == set(ENTRIES) - {'nlp_solve'}


def test_same_calls_as_the_parent(replay):
    parent, now = replay
    for name in sorted(parent):
        assert len(now[name]['calls']) == len(parent[name]['calls']) == 1, name
        for got, want in zip(now[name]['calls'], parent[name]['calls']):
            assert got['entry'] == want['entry'], name
            assert sorted(got['args']) == sorted(want['args']), name
            for k in want['args']:
                assert got['args'][k] == want['args'][k], (name, got['entry'], k)
        assert now[name] == parent[name], name                      # and what the caller made of the result: info keys, rows, result keys


GROUP = ('via', 'nlp_solve_groups_via'), ('knots', 'nlp_solve_groups_moving'), ('pairs', 'nlp_solve_groups_pairs'), ('field', 'nlp_solve_groups_wind')
HANDOUT = ('free_rows', 'nlp_solve_free'), ('via', 'nlp_solve_via'), ('knots', 'nlp_solve_moving'), ('field', 'nlp_solve_wind')
ENTRIES = tuple(e for _, e in GROUP + HANDOUT) + ('nlp_solve_groups', 'nlp_solve')
# the optional inputs each entry is handed (beside scen, W, h, n_ac of a group entry and the caller's own keywords)
TAKES = {'nlp_solve': (), 'nlp_solve_groups': (), 'nlp_solve_free': ('free_rows',), 'nlp_solve_wind': ('field', 't_start'),
         'nlp_solve_groups_wind': ('field', 't_start'), 'nlp_solve_groups_pairs': ('field', 't_start'),
         'nlp_solve_moving': ('knots', 'disc', 'field', 't_start'), 'nlp_solve_groups_moving': ('knots', 'disc', 'field', 't_start'),
         'nlp_solve_via': ('via', 'knots', 'disc', 'field', 't_start'), 'nlp_solve_groups_via': ('via', 'knots', 'disc', 'field', 't_start')}


class _Stub:
    """Any object with the nlp_solve* methods: each returns what it was called with."""

    def __getattr__(self, name):
        if name not in ENTRIES:
            raise AttributeError(name)
        return lambda *a, **kw: dict(called=name, a=a, kw=kw)


@pytest.mark.parametrize('group', [True, False])
def test_rule_first_match_wins(group):
    import d2dhip
    table = GROUP if group else HANDOUT
    values = dict(via='VIA', knots='KNOTS', pairs=True, field='FIELD', free_rows='FREE')
    for given in itertools.product([False, True], repeat=4):
        kw = {k: values[k] for (k, _), g in zip(table, given) if g}
        want = next((e for (k, e), g in zip(table, given) if g), 'nlp_solve_groups' if group else 'nlp_solve')
        if 'knots' in kw:
            kw['disc'] = 'DISC'
        if group:
            kw['n_ac'] = 3
        out = d2dhip.nlp_plan(_Stub(), 'SCEN', 'W', 0.1, t_start='T', bounds='B', opt_tol=1e-6, **kw)
        assert out['entry'] == out['called'] == want, (group, given)
        assert out['a'] == ('SCEN', 'W', 0.1)
        got = dict(out['kw'])
        assert got.pop('bounds') == 'B' and got.pop('opt_tol') == 1e-6 and (got.pop('n_ac') == 3 if group else 'n_ac' not in got)
        assert sorted(got) == sorted(TAKES[want]), (want, got)
        for k in TAKES[want]:
            assert got[k] == ('T' if k == 't_start' else kw.get(k)), (want, k)          # (an input that was not given: None)


def test_rule_defaults():
    """Nothing given: nlp_solve / nlp_solve_groups with no optional input; a field without a start time starts the hand-out entry at 0."""
    import d2dhip
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1)['kw'] == {} and d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1)['entry'] == 'nlp_solve'
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, n_ac=1)['kw'] == {'n_ac': 1}
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, field='F')['kw'] == {'field': 'F', 't_start': 0.0}
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, n_ac=2, pairs=True)['kw'] == {'n_ac': 2, 'field': None, 't_start': None}


def test_default_pair_masks():
    import numpy as np
    import torch
    import d2dhip
    from d2d.multiopty_utils import default_pair_masks
    dsc = torch.full((6, d2dhip.SCEN_STRIDE), 7.0, dtype=torch.float64)
    default_pair_masks(dsc, 3, torch.tensor([True, False]))
    assert dsc[:, d2dhip.SC_PMASK].tolist() == [2.0, 1.0, 7.0, 0.0, 0.0, 7.0]
    assert (np.delete(dsc.numpy(), d2dhip.SC_PMASK, axis=1) == 7.0).all()
    default_pair_masks(dsc, 2, True)
    assert dsc[:, d2dhip.SC_PMASK].tolist() == [2.0, 1.0] * 3
