"""The planners' choice among the collocation entries (d2dhip.nlp_plan), without a GPU.

1. Same routing as before the ladders were folded: tests/golden/make_nlp_dispatch_golden.py drives Problem.solve (through both
   planners) and plan_batch over a recording stand-in of the context; tests/golden/nlp_dispatch_parent.json is what it recorded at
   the commit before the fold.  Every call -- entry, rows, tables, options -- must be the same.
2. The rule itself: nlp_plan with every combination of the optional inputs lands on the entry its table names, and hands it the
   inputs that entry takes.
3. The same for the entries added since (hard discs, hard moving discs, the geofence, the free step beside them), deconflict= and
   W0='dubins': nlp_dispatch_abi129.json, recorded at the commit before nlp_plan and plan_batch were restated as tables
   (d2dhip.plan.ENTRIES / REFUSES).
4. Every refusal and every route, exhaustively: nlp_dispatch_refusals.json holds the outcome, at that commit, of nlp_plan for every
   subset of its 13 optional inputs and of plan_batch for backend x n_ac x every subset of its 10 optional features."""
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


def test_the_newer_families_make_the_same_calls(maker):
    """nlp_dispatch_abi129.json, call by call: entry, every argument by hash, result keys, returned scen."""
    with open(os.path.join(GOLD, 'nlp_dispatch_abi129.json')) as f:
        parent = json.load(f)
    now = json.loads(json.dumps(maker.collect('abi129')))
    assert sorted(now) == sorted(parent) and len(parent) >= 50
    for name in sorted(parent):
        assert [c['entry'] for c in now[name]['calls']] == [c['entry'] for c in parent[name]['calls']], name
        for got, want in zip(now[name]['calls'], parent[name]['calls']):
            assert sorted(got['args']) == sorted(want['args']), name
            for k in want['args']:
                assert got['args'][k] == want['args'][k], (name, got['entry'], k)
        assert now[name] == parent[name], name
    # with the first file every entry nlp_plan can choose is reached through a planner or plan_batch -- but nlp_solve, which neither
    # ever chooses (the rule's own test below reaches it)
    with open(os.path.join(GOLD, 'nlp_dispatch_parent.json')) as f:
        both = list(parent.values()) + list(json.load(f).values())
    import d2dhip.plan
    assert len(d2dhip.plan.ENTRIES) == 16
    assert {c['entry'] for v in both for c in v['calls']} >= {row[0] for row in d2dhip.plan.ENTRIES} - {'nlp_solve'}


def test_every_subset_of_the_inputs_ends_as_it_did(maker):
    """nlp_dispatch_refusals.json: all 8192 subsets of nlp_plan's optional inputs and all 4096 (+1) calls of plan_batch end at the same
    entry with the same inputs, or raise the same exception with the same text."""
    with open(os.path.join(GOLD, 'nlp_dispatch_refusals.json')) as f:
        parent = json.load(f)
    now = maker.refusals()
    assert len(parent['nlp_plan']) == 2 ** len(maker.PLAN_INPUTS) == 8192 and len(parent['plan_batch']) == 4 * 2 ** len(maker.BATCH_FEATURES) + 1
    for what in ('nlp_plan', 'plan_batch'):
        assert len(now[what]) == len(parent[what])
        for i, (got, want) in enumerate(zip(now[what], parent[what])):
            assert now['outcomes'][got] == parent['outcomes'][want], (what, i)
    ends = [parent['outcomes'][i] for i in parent['nlp_plan']]
    assert sum('entry' in o for o in ends) == 328 and sum(o.get('raises') == 'NotImplementedError' for o in ends) == 7832
    assert sum(o.get('raises') == 'ValueError' for o in ends) == 32 and len({o['message'] for o in ends if 'raises' in o}) == 25
    import d2dhip.plan
    assert {o['entry'] for o in ends if 'entry' in o} == {row[0] for row in d2dhip.plan.ENTRIES}         # all sixteen


def test_plan_batch_docstring_table_is_the_table():
    """The compatibility table at the end of plan_batch's docstring says what PLAN_BATCH_REFUSES (and free_time's two checks) refuse."""
    import full_sim as fs
    lines = fs.plan_batch.__doc__.split('with the fit backend:\n')[1].splitlines()
    doc = {ln.split()[0]: tuple(ln.split(None, 1)[1].split(', ')) for ln in lines}
    assert doc == {'free_time': ('n_ac > 1', 'windfield', 'moving', 'via'), **{k: v[0] for k, v in fs.PLAN_BATCH_REFUSES.items()}}
    assert set(fs.PLAN_BATCH_FIT) == set(doc) | {'windfield', 'moving', 'via'}


def test_the_module_table_is_the_pinned_one():
    """d2dhip.plan.ENTRIES against the literal tables below, for the ten entries they name: precedence, launch shape, naming input, and
    the inputs handed."""
    from d2dhip.plan import ENTRIES as rows
    by = {entry: (groups, named, tuple(k for k in pos if k != 'n_ac') + tuple(takes)) for entry, groups, named, pos, takes in rows}
    assert len(by) == len(rows) == 16
    for entry in ENTRIES:
        assert by[entry][2] == TAKES[entry], entry
    for table, groups in ((GROUP, True), (HANDOUT, False)):
        tail = [(named, entry) for entry, g, named, _, _ in rows if g == groups and entry in ENTRIES]
        assert tuple(tail) == table + ((None, 'nlp_solve_groups' if groups else 'nlp_solve'),)


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
