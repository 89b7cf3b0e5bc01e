"""tests/helper_cases.py says what it claims (no GPU): the exact wrap edges are in the formation cases and the oracle maps them to
pi, pi, 0; a dense-B case leaves (-pi, pi] after the single wrap; next to nothing is dropped for nearness to a wrap threshold; the
inputs stay where the maps are well conditioned; every builder is deterministic."""
import numpy as np
import pytest

import helper_cases as HC
from oracle import fit as F, sim as S


@pytest.fixture(scope='module')
def dcf():
    return HC.dcf_cases()


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def test_probe_indices_cover_both_sides_of_every_boundary():
    for n in HC.NS + HC.NS_LQR:
        idx = HC.probe_indices(n)
        assert len(idx) >= min(n, 8) and idx[0] == 0 and idx[-1] == n - 1 and len(set(idx)) == len(idx)
        for b in range(64, n, 64):
            assert b - 1 in idx and b in idx


def test_exact_wrap_edges_are_present_and_the_oracle_maps_them_to_pi_pi_0(dcf):
    assert HC.EDGE_UNWRAPPED == (np.pi, -np.pi, 2 * np.pi)
    seen = set()
    for case in dcf:
        assert bool(case['edges']) == (not case['dense'] and case['n_ac'] >= 2 and case['n_form'] >= 3)
        nm = case['n_ac'] - 1
        for f, kind in case['edges']:
            assert not case['z_des'].any() and np.array_equal(case['B'], S.construct_b_matrix(case['n_ac']))
            raw = case['raw'][f]
            assert raw[0] == HC.EDGE_UNWRAPPED[kind] and np.isin(raw, (0.0,) + HC.EDGE_UNWRAPPED).all()      # bit for bit
            want = (np.pi, np.pi, 0.0)[kind]
            eth = case['eth_deg'][f * nm:(f + 1) * nm]
            assert eth[0] == np.rad2deg(want) and (want == 0.0 or eth[0] == 180.0)
            # and the control it gives: -kr B e with e = (want, 0, ..)
            e = np.zeros(nm); e[0] = want
            np.testing.assert_array_equal(case['U_r'][f * case['n_ac']:(f + 1) * case['n_ac']], -case['kr'] * (case['B'] @ e))
            seen.add(kind)
    assert seen == {0, 1, 2}
    # the sign of zero that makes atan2 answer -pi survives the planar packing
    c, p = HC.edge_formation(2, 2)
    assert np.signbit(p[1, 0]) and not np.signbit(c[0, 1]) and np.arctan2(p[1, 0] - c[0, 1], p[0, 0] - c[0, 0]) == -np.pi


def test_a_dense_case_stays_outside_after_one_wrap_and_almost_nothing_is_dropped(dcf):
    dense = [c for c in dcf if c['dense']]
    assert sorted({c['n_ac'] for c in dense}) == list(HC.DENSE_N_ACS) and sorted({c['n_form'] for c in dense}) == list(HC.N_FORMS)
    beyond = sum(int((np.abs(c['raw']) > 3 * np.pi).any(axis=1).sum()) for c in dense)
    assert beyond >= 1
    outside = sum(int((np.abs(c['eth_deg']) > 180.0).sum()) for c in dense)
    assert outside >= 1                                       # the oracle's answer itself is outside (-180, 180] there
    drawn, dropped = sum(c['drawn'] for c in dense), sum(c['dropped'] for c in dense)
    assert drawn >= sum(c['n_form'] for c in dense) and dropped < 0.01 * drawn
    print('dense B: %d of %d formations beyond 3 pi before the wrap, %d answers outside (-180, 180], %d of %d dropped'
          % (beyond, sum(c['n_form'] for c in dense), outside, dropped, drawn))
    for c in dcf:                                             # no random formation sits within NEAR_PI of a wrap threshold
        skip = {f for f, _ in c['edges']}
        keep = [f for f in range(c['n_form']) if f not in skip]
        if c['n_ac'] > 1:
            assert np.abs(np.abs(c['raw'][keep]) - np.pi).min() > HC.NEAR_PI


def test_formation_cases_cover_the_sizes(dcf):
    inc = {(c['n_form'], c['n_ac']) for c in dcf if not c['dense']}
    assert inc == {(nf, na) for nf in HC.N_FORMS for na in HC.N_ACS}
    for c in dcf:
        N = c['n_form'] * c['n_ac']
        assert c['centres'].shape == (2, N) and c['pos'].shape == (2, N) and c['U_r'].shape == (N,)
        assert c['eth_deg'].shape == (c['n_form'] * (c['n_ac'] - 1),) and c['B'].shape == (c['n_ac'], c['n_ac'] - 1)


def test_conditioning_bounds_hold():
    windy = 0
    cases = [HC.flatness_case(v, n) for v in (0, 1) for n in HC.NS]
    for c in cases:
        n = c['n']
        assert c['Yref'].shape == (8, n)
        va = np.hypot(c['Yref'][2] - c['w'][0], c['Yref'][3] - c['w'][1])
        assert HC.V_AIR[0] <= va.min() and va.max() <= HC.V_AIR[1]
        assert HC.V_AIR[0] <= c['X'][4].min() and c['X'][4].max() <= HC.V_AIR[1]
        assert np.abs(c['X'][3]).max() < 1.0 and np.isfinite(c['U']).all() and np.isfinite(c['Xdot']).all()
        windy += int(any(c['w']) and c['tau_phi'] != 0.01 and c['tau_v'] != 1.0)
    assert 2 * windy >= len(cases)
    lagged = 0
    for n in HC.NS:
        c = HC.cont_jac_case(n)
        assert np.abs(c['Xr'][3]).max() < 1.0 and HC.V_AIR[0] <= c['Xr'][4].min() and c['Xr'][4].max() <= HC.V_AIR[1]
        assert c['A'].shape == (25, n) and c['B'].shape == (10, n)
        lagged += int(c['tau_phi'] != 0.01 and c['tau_v'] != 1.0)
        g = HC.gvf_case(n)
        assert np.hypot(g['X'][0] - g['c'][0], g['X'][1] - g['c'][1]).min() >= HC.GVF_MIN_DIST * (1 - 1e-12)
        assert HC.V_AIR[0] <= g['X'][4].min() and g['X'][4].max() <= HC.V_AIR[1] and np.isfinite(g['U']).all()
        assert g['e'].shape == (n,) and g['nvec'].shape == (2, n) and g['H'].shape == (4, n) and g['U'].shape == (3, n)
    assert 2 * lagged >= len(HC.NS)


def test_fit_case_has_wind_rows_and_is_the_oracle():
    K, S_ = 50, 6
    dur = F.planner_timing(0, 4.9, 10)[2]
    s = 0.1 / K
    b = F.FitBasis(S_, K, dur, (0.02 ** 2, s * 5.0, s / F.G_ACC ** 2))
    for B in HC.FIT_BS[:4]:
        c = HC.fit_case(b, B)
        sc = c['scen']
        assert sc.shape == (B, F.SCEN_STRIDE) and (np.hypot(sc[:, F.SC_WX], sc[:, F.SC_WY]) > 0).any()
        assert c['xy'].shape == (B, 2, K) and c['z'].shape == (B, 2, S_, 8) and c['Y'].shape == (B, 6, K) and c['Xs'].shape == (B, 5, K)
        i = B - 1
        np.testing.assert_array_equal(c['q_wp'][i], F.initial_guess(b, sc[i]))                  # the oracle's own waypoints
        np.testing.assert_array_equal(c['Y'][i, 2], F.flat_outputs(b, sc[i], c['q'][i])[1, 0])   # plane 2 = xd
        assert c['Xs'][:, 4].min() > 1.0                       # airspeed away from the singularity of the flatness map
    _same(HC.fit_case(b, 3), HC.fit_case(b, 3))
    # the lattice rows: no dog-leg (the leg is longer than vref x duration) and integer waypoints from end to end
    for K2 in (50, 57, 121):
        b2 = b if K2 == 50 else F.FitBasis(S_, K2, (K2 - 1) / 10.0, (0.02 ** 2, 0.1 / K2 * 5.0, 0.1 / K2 / F.G_ACC ** 2))
        lat = HC.fit_lattice_case(b2, 5)
        sc = lat['scen']
        assert (np.hypot(sc[:, F.SC_X1] - sc[:, F.SC_X0], sc[:, F.SC_Y1] - sc[:, F.SC_Y0]) > sc[:, F.SC_VREF] * b2.duration).all()
        assert lat['wp'].shape == (5, 2, K2) and np.array_equal(lat['wp'], np.round(lat['wp'])) and np.abs(lat['wp']).max() < 2.0 ** 40
        assert np.array_equal(lat['wp'][:, 0, 0], sc[:, F.SC_X0]) and np.array_equal(lat['wp'][:, 1, -1], sc[:, F.SC_Y1])
        assert (np.abs(np.diff(lat['wp'], axis=2)).max(axis=(1, 2)) > 0).all()
        np.testing.assert_array_equal(lat['q_wp'][4], F.initial_guess(b2, sc[4]))
    _same(HC.fit_lattice_case(b, 5), HC.fit_lattice_case(b, 5))


def test_builders_are_deterministic(dcf):
    for n in (1, 65, 257):
        for v in (0, 1):
            _same(HC.flatness_case(v, n), HC.flatness_case(v, n))
        _same(HC.cont_jac_case(n), HC.cont_jac_case(n))
        _same(HC.gvf_case(n), HC.gvf_case(n))
    for n in (1, 65):
        _same(HC.lqr_case(n), HC.lqr_case(n))
    for a, b in zip(dcf, HC.dcf_cases()):
        _same(a, b)
