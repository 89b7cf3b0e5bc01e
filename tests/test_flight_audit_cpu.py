"""The flight audit without a GPU: the CPU statement tests/flight_audit_ref.py against a brute-force minimum and against known
answers, its refusals, and the host plumbing (the `audit=` argument is off by default, the header carries the entry)."""
import inspect
import os
import re

import numpy as np
import pytest

import flight_audit_ref as FA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_history = FA.synthetic_history


@pytest.mark.parametrize('n_ac', [2, 3, 5])
def test_closed_form_against_brute_force(n_ac):
    n_rows, sub, dt = 7, 2000, 0.1
    X = _history(3, n_ac, n_rows, seed=n_ac, span=10.0)
    out = FA.audit(X, n_ac, dt)
    s = np.arange(sub + 1) / sub
    for d in range(X.shape[2]):
        f = d // n_ac
        brute = np.inf
        for j in range(n_ac):
            if j == d % n_ac:
                continue
            P = X[:, :2, f * n_ac + j] - X[:, :2, d]
            for i in range(n_rows - 1):
                q = P[i][None] + s[:, None] * (P[i + 1] - P[i])[None]
                brute = min(brute, np.hypot(q[:, 0], q[:, 1]).min())
        ref = out['sep_dist'][d]
        assert ref <= brute + 1e-12                  # never larger (1e-12: the brute force's own rounding at |q| <= 1e2)
        # a sample lies within |d| / (2 sub) of s*, so the brute force exceeds the minimum by at most |d|^2 / (8 sub^2 dist): 1e-5 here
        assert brute - ref <= 1e-5
        # the reported time and partner give the reported distance
        assert abs(FA.pair_distance(X, n_ac, dt, d, out['sep_partner'][d], out['sep_time'][d]) - ref) <= 1e-12


def _crossing(n_rows=5, v=30.0, dt=0.1, offset=0.5):
    """Two aircraft on perpendicular legs through the origin, both there at row `offset` + (n_rows - 1) // 2: between two rows."""
    i = np.arange(n_rows) - ((n_rows - 1) // 2 + offset)
    X = np.zeros((n_rows, 5, 2))
    X[:, 0, 0] = v * dt * i                      # eastbound along y = 0
    X[:, 1, 1] = v * dt * i                      # northbound along x = 0
    X[:, 4] = v
    return X, dt


def test_crossing_between_rows():
    X, dt = _crossing()
    out = FA.audit(X, 2, dt, d_safe=1.0)
    step = 30.0 * dt
    assert np.all(out['sep_dist'] <= 1e-12) and list(out['sep_partner']) == [1, 0]
    np.testing.assert_allclose(out['sep_time'], 2.5 * dt, rtol=0, atol=1e-12)
    # the rows see |d| / sqrt 2, |d| = 3 m an aircraft's step: both are half a step from the crossing
    np.testing.assert_allclose(FA.rowwise_min(X, 2), step / np.sqrt(2), rtol=1e-12)
    assert list(out['sep_count']) == [0, 0]          # no ROW is closer than 1 m: the count is row-wise


def test_tangent_to_a_static_disc_between_rows():
    n_rows, dt, r = 4, 0.5, 3.0
    X = np.zeros((n_rows, 5, 1))
    X[:, 0, 0] = 10.0 * (np.arange(n_rows) - 1.25)   # along y = 0, abeam the disc a quarter into the segment 1 -> 2
    static = np.array([[[0.0, r, r], [0.0, 0.0, -1.0], [100.0, 0.0, 2.0]]])     # tangent disc, an absent one, a far one
    out = FA.audit(X, 1, dt, static=static, t_start=7.0)
    assert abs(out['stat_clear'][0, 0]) <= 1e-12 and abs(out['stat_time'][0, 0] - (7.0 + 1.25 * dt)) <= 1e-12
    assert out['stat_count'][0, 0] == 0
    assert out['stat_clear'][1, 0] == np.inf and np.isnan(out['stat_time'][1, 0]) and out['stat_count'][1, 0] == 0
    assert abs(out['stat_clear'][2, 0] - (100.0 - 17.5 - 2.0)) <= 1e-12 and abs(out['stat_time'][2, 0] - (7.0 + 3 * dt)) <= 1e-12
    # no partner: nothing seen
    assert out['sep_dist'][0] == np.inf and out['sep_partner'][0] == -1 and np.isnan(out['sep_time'][0]) and out['sep_count'][0] == 0


def test_moving_disc_on_a_parallel_course():
    n_rows, dt, t0 = 6, 0.2, 3.0
    X = np.zeros((n_rows, 5, 1))
    X[:, 0, 0] = 12.0 * dt * np.arange(n_rows)
    knots = np.array([[[[t0, 0.0, 5.0], [t0 + 10.0, 120.0, 5.0]]]])            # the same 12 m/s, 5 m abeam
    disc = np.array([[[2.0, 0.0]]])
    out = FA.audit(X, 1, dt, t_start=t0, knots=knots, disc=disc)
    assert abs(out['mov_clear'][0, 0] - 3.0) <= 1e-12 and out['mov_count'][0, 0] == 0
    assert abs(out['mov_time'][0, 0] - t0) <= 1e-12 or out['mov_clear'][0, 0] < 3.0        # constant: the earliest time unless rounding found less
    for i in range(n_rows):
        assert abs(FA.disc_clearance(X, dt, 0, FA.mov_centres(knots[0], t0, n_rows, dt)[0], 2.0, t0 + i * dt, t0) - 3.0) <= 1e-12


def test_refusals_and_valid_rows():
    X = _history(3, 2, 6, seed=11)
    X[2, 2, :] = np.nan                              # psi is never read
    base = FA.audit(X, 2, 0.1, d_safe=5.0)
    assert (base['status'] == 0).all()
    Xb = X.copy()
    Xb[4, 1, 3] = np.nan                             # formation 1, aircraft 1
    out = FA.audit(Xb, 2, 0.1, d_safe=5.0)
    assert list(out['status']) == [0, FA.NONFINITE, 0]
    assert np.isnan(out['sep_dist'][2:4]).all() and np.isnan(out['v_max'][2:4]).all() and (out['sep_count'][2:4] == -1).all()
    assert (out['sep_partner'][2:4] == -1).all()
    for k in ('sep_dist', 'sep_time', 'sep_partner', 'sep_count', 'phi_max', 'v_min', 'v_max'):
        assert np.array_equal(out[k][[0, 1, 4, 5]], base[k][[0, 1, 4, 5]])
    # ... unless the row is behind the formation's valid rows: rows = 0 / 1 / 2 for the three formations
    out = FA.audit(Xb, 2, 0.1, rows=np.array([0, 1, 2]), d_safe=5.0, t_start=np.array([0.0, 5.0, 9.0]))
    assert (out['status'] == 0).all()
    assert (out['sep_dist'][:2] == np.inf).all() and np.isnan(out['sep_time'][:2]).all() and (out['sep_partner'][:2] == -1).all()
    assert (out['phi_max'][:2] == -np.inf).all() and (out['v_min'][:2] == np.inf).all() and (out['sep_count'][:2] == 0).all()
    d1 = np.hypot(*(Xb[0, :2, 2] - Xb[0, :2, 3]))    # one row: the row itself
    np.testing.assert_allclose(out['sep_dist'][2:4], d1, rtol=1e-15)
    assert (out['sep_time'][2:4] == 5.0).all()
    two = FA.audit(X[:2, :, 4:6], 2, 0.1, d_safe=5.0, t_start=9.0)
    for k in ('sep_dist', 'sep_time', 'sep_partner', 'sep_count', 'phi_max'):
        assert np.array_equal(out[k][4:6], two[k])
    # a start time that is not finite, a track whose knot times do not increase
    knots = np.tile(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 0.0]]), (3, 1, 1, 1))
    disc = np.tile(np.array([[1.0, 0.0]]), (3, 1, 1))
    knots[2, 0, 2, 0] = 1.0
    out = FA.audit(X, 2, 0.1, t_start=np.array([0.0, np.inf, 0.0]), knots=knots, disc=disc)
    assert list(out['status']) == [0, FA.BAD_TSTART, FA.BAD_TRACK]
    assert np.isfinite(out['mov_clear'][0, :2]).all() and np.isnan(out['mov_clear'][0, 2:]).all() and (out['mov_count'][0, 2:] == -1).all()


def test_ties():
    # two partners placed symmetrically about aircraft 0's track: the same distance at the same time, the smaller index wins
    X = np.zeros((3, 5, 3))
    X[:, 0, 0] = [-1.0, 0.0, 1.0]
    X[:, 1, 1], X[:, 1, 2] = 2.0, -2.0
    out = FA.audit(X, 3, 1.0)
    assert out['sep_partner'][0] == 1 and out['sep_dist'][0] == 2.0 and out['sep_time'][0] == 1.0
    # the same minimum at two rows: the earlier time
    Y = np.zeros((5, 5, 2))
    Y[:, 0, 1] = [3.0, 1.0, 3.0, 1.0, 3.0]
    out = FA.audit(Y, 2, 0.5)
    assert (out['sep_dist'] == 1.0).all() and (out['sep_time'] == 0.5).all()


def test_audit_is_off_by_default_and_the_header_carries_the_entry():
    import d2dhip
    import full_sim
    for fn in (full_sim.full_sim_phases_batch, full_sim.CircularFormationGVF_batch, full_sim.implement_controller_batch):
        assert inspect.signature(fn).parameters['audit'].default is None
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 117
    assert 'd2d_flight_audit' in d2dhip.EXPORTS and re.search(r'\bint d2d_flight_audit\(', hdr)
    val = lambda name: int(re.search(r'#define %s (\d+)' % name, hdr).group(1))       # noqa: E731
    assert (d2dhip.AUDIT_NONFINITE, d2dhip.AUDIT_BAD_TSTART, d2dhip.AUDIT_BAD_TRACK) == (FA.NONFINITE, FA.BAD_TSTART, FA.BAD_TRACK) \
        == tuple(val('D2D_AUDIT_' + k) for k in ('NONFINITE', 'BAD_TSTART', 'BAD_TRACK'))
    # d2d_audit_out: one pointer per name, in the header's order
    body = re.search(r'typedef struct \{([^}]*)\} d2d_audit_out;', hdr).group(1)
    assert tuple(re.findall(r'\*(\w+);', body)) == d2dhip.AUDIT_OUT == tuple(k for k, _ in d2dhip.AuditOut._fields_)
    body = re.search(r'typedef struct \{([^}]*)\} d2d_audit_params;', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)).group(1)
    names = [n.strip() for decl in re.findall(r'(?:int32_t|double) ([^;]+);', body) for n in decl.split(',')]
    assert names == [k for k, _ in d2dhip.AuditParams._fields_]
    with pytest.raises(ValueError, match="'X' must be in record"):
        full_sim.implement_controller_batch(np.arange(3) * 0.1, np.zeros((3, 1)), np.zeros((3, 1)), (0., 0.), np.zeros((1, 5)), record=('U',),
                                            audit=True)
