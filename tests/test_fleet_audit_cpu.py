"""The fleet audit without a GPU: the header and the binding agree, the CPU statement tests/fleet_audit_ref.py reduces to the
in-formation statement when every aircraft is its own formation, its worlds, look radius and refusals, and the host side of the
`audit=dict(fleet=...)` hook."""
import ctypes
import os
import re

import numpy as np
import pytest

import fleet_audit_ref as FL
import flight_audit_ref as FA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'd2d.h')).read()


def test_the_header_carries_the_entry():
    import d2dhip
    hdr = _header()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 123
    assert re.search(r'\bint d2d_fleet_audit\(', hdr) and re.search(r'\bint64_t d2d_fleet_audit_workspace\(', hdr)
    assert 'd2d_fleet_audit' in d2dhip.EXPORTS and 'd2d_fleet_audit_workspace' in d2dhip.EXPORTS
    val = lambda name: int(re.search(r'#define %s (\d+)' % name, hdr).group(1))       # noqa: E731
    assert (d2dhip.FLEET_NONFINITE, d2dhip.FLEET_STEP, d2dhip.FLEET_BAD_ROW0, d2dhip.FLEET_RANGE) == (FL.NONFINITE, FL.STEP, FL.BAD_ROW0, FL.RANGE) \
        == tuple(val('D2D_FLEET_' + k) for k in ('NONFINITE', 'STEP', 'BAD_ROW0', 'RANGE'))


def test_struct_layouts_match_the_header():
    import d2dhip
    hdr = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} d2d_fleet_out;', hdr).group(1)
    assert tuple(re.findall(r'\*(\w+);', body)) == d2dhip.FLEET_OUT == tuple(k for k, _ in d2dhip.FleetOut._fields_)
    assert ctypes.sizeof(d2dhip.FleetOut) == 5 * 8
    body = re.search(r'typedef struct \{([^}]*)\} d2d_fleet_params;', hdr).group(1)
    decls = re.findall(r'(int32_t|double) ([^;]+);', body)
    names = [n.strip() for _, decl in decls for n in decl.split(',')]
    assert names == [k for k, _ in d2dhip.FleetParams._fields_]
    size = sum((4 if t == 'int32_t' else 8) * len(decl.split(',')) for t, decl in decls)
    assert size == ctypes.sizeof(d2dhip.FleetParams) == 6 * 4 + 4 * 8
    types = [ctypes.c_int32 if t == 'int32_t' else ctypes.c_double for t, decl in decls for _ in decl.split(',')]
    assert types == [t for _, t in d2dhip.FleetParams._fields_]
    # the sizes of the older structures are as they were
    assert ctypes.sizeof(d2dhip.AuditParams) == 6 * 4 + 3 * 8 and ctypes.sizeof(d2dhip.AuditOut) == 17 * 8


@pytest.mark.parametrize('N,n_rows', [(2, 1), (7, 2), (23, 9), (64, 5)])
def test_one_aircraft_per_formation_is_the_in_formation_statement(N, n_rows):
    """n_ac = 1 and d_look = inf: every other aircraft is a partner, as in flight_audit_ref.audit with n_ac = N."""
    X = FA.synthetic_history(1, N, n_rows, seed=N, span=30.0)
    a = FA.audit(X, N, 0.25)
    b = FL.audit(X, 1, 0.25, np.inf, 1e9)
    assert (b['status'] == 0).all()
    assert np.array_equal(b['near_dist'], a['sep_dist']) and np.array_equal(b['near_partner'], a['sep_partner'])
    assert np.array_equal(b['near_time'], a['sep_time'])


def test_formations_worlds_and_the_look_radius():
    # formations of two; A = (0, 0), its partner 1 m away (never reported), formation 1 at 5 m, formation 2 at 7 m
    X = np.zeros((3, 5, 6))
    X[:, 0, 1], X[:, 0, 2], X[:, 0, 3], X[:, 1, 4], X[:, 1, 5] = 1.0, 5.0, 50.0, 7.0, 70.0
    out = FL.audit(X, 2, 0.5, 10.0, 1.0, d_safe=6.0)
    assert out['near_partner'][0] == 2 and out['near_dist'][0] == 5.0 and out['near_time'][0] == 0.0 and out['near_count'][0] == 3
    assert out['near_partner'][1] == 2 and out['near_dist'][1] == 4.0
    assert out['near_dist'][3] == np.inf and out['near_partner'][3] == -1 and np.isnan(out['near_time'][3]) and out['near_count'][3] == 0
    # formation 1 in another world: A sees formation 2
    out = FL.audit(X, 2, 0.5, 10.0, 1.0, world=np.array([0, 1, 0]), d_safe=6.0)
    assert out['near_partner'][0] == 4 and out['near_dist'][0] == 7.0 and out['near_count'][0] == 0 and out['near_partner'][2] == -1
    # exactly d_look away is not seen: strictly below
    out = FL.audit(X, 2, 0.5, 5.0, 1.0)
    assert out['near_partner'][0] == -1 and out['near_dist'][1] == 4.0
    # the common clock: formation 1 placed three rows later meets nobody (rows 3 .. 5 against 0 .. 2); two rows later, one row
    out = FL.audit(X, 2, 0.5, 10.0, 1.0, row0=np.array([0, 3, 0]))
    assert (out['status'] == 0).all() and out['near_partner'][0] == 4 and out['near_partner'][2] == -1
    out = FL.audit(X, 2, 0.5, 10.0, 1.0, row0=np.array([0, 2, 0]), d_safe=6.0)
    assert out['near_partner'][0] == 2 and out['near_time'][0] == 1.0 and out['near_time'][2] == 1.0 and out['near_count'][0] == 1


def test_a_refused_formation_is_absent_for_the_others():
    X = FA.synthetic_history(4, 2, 6, seed=3, span=8.0)
    kw = dict(d_safe=9.0)
    rest = FL.audit(np.delete(X, [2, 3], axis=2), 2, 0.5, 30.0, 4.3, **kw)
    for bit, edit in ((FL.NONFINITE, lambda Y: Y.__setitem__((4, 1, 3), np.nan)), (FL.STEP, lambda Y: Y.__setitem__((slice(3, None), 0, 2), Y[3:, 0, 2] + 5.0)),
                      (FL.RANGE, lambda Y: Y.__setitem__((slice(None), 0, slice(2, 4)), Y[:, 0, 2:4] + 1e13))):
        Y = X.copy()
        edit(Y)
        out = FL.audit(Y, 2, 0.5, 30.0, 4.3, **kw)
        assert list(out['status']) == [0, bit, 0, 0]
        assert np.isnan(out['near_dist'][2:4]).all() and (out['near_partner'][2:4] == -1).all() and (out['near_count'][2:4] == -1).all()
        keep = [0, 1, 4, 5, 6, 7]
        assert np.array_equal(out['near_dist'][keep], rest['near_dist']) and np.array_equal(out['near_count'][keep], rest['near_count'])
        assert np.array_equal(out['near_partner'][keep], np.where(rest['near_partner'] >= 2, rest['near_partner'] + 2, rest['near_partner']))
    out = FL.audit(X, 2, 0.5, 30.0, 4.3, row0=np.array([0, -1, 0, 1]), g_rows=6)
    assert list(out['status']) == [0, FL.BAD_ROW0, 0, FL.BAD_ROW0]
    Y = X.copy(); Y[4:, :, 2:4] = np.nan                             # behind the valid rows: never read
    assert (FL.audit(Y, 2, 0.5, 30.0, 4.3, rows=np.array([6, 4, 6, 6]))['status'] == 0).all()


def test_the_hook_refuses_a_start_off_the_row_grid_by_name():
    import full_sim
    assert list(full_sim.fleet_row0([2.0, 2.5, 3.0 + 1e-12], 0.25)) == [0, 2, 4]
    with pytest.raises(ValueError, match='formation 2 '):
        full_sim.fleet_row0([2.0, 2.5, 3.1, 2.6], 0.25)
    with pytest.raises(ValueError, match='d_look and step_max'):
        full_sim._fleet_audit(None, dict(fleet=dict(d_look=5.0)), None, 1, 0.1, 1)
    assert full_sim._fleet_audit(None, dict(d_safe=1.0), None, 1, 0.1, 1) is None and full_sim._fleet_audit(None, True, None, 1, 0.1, 1) is None
    assert full_sim._audit_kw(None, dict(fleet=dict(d_look=1.0, step_max=1.0)), 1, ('fleet',)) == dict(d_safe=0.0, err_tol=np.inf)
    with pytest.raises(ValueError, match='unknown keys'):
        full_sim._audit_kw(None, dict(fleet={}), 1, ())
