"""GPU: the three-phase mission when the wind must be learned -- full_sim.full_sim_phases_batch(windfield=F, wind_estimate=E) flies
the unknown field F, fits F^ to its own phase 1 on the device and plans the transition in -F^ -- against the mission that is handed
the truth and the one that plans in no wind at all."""
import numpy as np
import pytest

import nlp_groups_wind_ref as G
import wind_fit_ref as WF

pytestmark = pytest.mark.gpu


def _estimator(**kw):
    """A grid over what phase 1 of G.mission_inputs() flies: circles of radius 60 m around x in [0, 25], y in [-100, -20], until about
    134 s; 10 s knots in time (the field has a kink at 100 s), every fourth row kept (dt_row = 0.2 s)."""
    from d2d.wind import WindEstimator
    return WindEstimator(np.arange(-120.0, 161.0, 70.0), np.arange(-220.0, 101.0, 80.0), np.arange(0.0, 190.1, 10.0),
                         **dict(dict(lam=1e-2, mu=1e-6, rec_stride=4), **kw))


def test_the_mission_plans_in_the_field_it_identified():
    """Three formations of four aircraft, F = G.mission_field() (the committed field at its committed strength: about 1.17 m/s of head
    wind when phase 1 ends), three ways: planned in the true field, in the estimate, and in no wind -- the last through the same path
    with an estimator whose pull towards its prior 0 is overwhelming (mu = 1e12), so that it plans in F^ = 0 while the plant still
    flies F.  info['wind_fit'] is present; F^ is within twice the recorded unsteady tolerance (wind_fit_ref.RECOVERY_ERR['gust']) of F
    along phase 1; the phase-2 tracking error (flight_audit err_max) of the estimated-wind mission is closer to the true-wind
    mission's than the no-wind mission's is; and wind_estimate=None is the existing mission bit for bit."""
    import torch
    import d2dhip as D
    import full_sim as fs
    import multi_opt_planner as mop
    F = G.mission_field()
    n_ac, c, X1_f, X2_f, X0B, _ = G.mission_inputs()
    cB = np.stack([c, c, c])
    r, v, t_opt = 60, 15, 6
    dctx = D.default_context()
    run = lambda **kw: fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, X0=X0B, windfield=F, audit=True, **kw)   # noqa: E731
    true = run()
    est = run(wind_estimate=_estimator())
    none = run(wind_estimate=_estimator(mu=1e12))
    same = run(wind_estimate=None)
    dctx.sync()
    # None is today's path
    for k in ('Xs', 'cost', 'status'):
        assert torch.equal(true['plan'][k], same['plan'][k])
    assert torch.equal(true['phase2']['X'], same['phase2']['X']) and 'wind_fit' not in same and 'wind_fit' not in true
    # the flights of phase 1 are the same flight: the estimator only listens
    assert torch.equal(true['phase1']['X_final'], est['phase1']['X_final']) and torch.equal(true['phase1']['stop_row'], est['phase1']['stop_row'])
    info = est['wind_fit']
    stats = dict(zip(D.WINDFIT_STATS, info['stats'].cpu().numpy()))
    stop = est['phase1']['stop_row'].cpu().numpy()
    rows = (np.minimum(stop, len(est['phase1']['time'])) + 3) // 4
    assert stats['used'] + stats['nonfinite'] + stats['outside'] + stats['over'] == float(((rows - 1) * n_ac).sum())
    assert stats['used'] >= 0.99 * ((rows - 1) * n_ac).sum() and stats['cg_resid'] <= 1e-10
    assert info['support'].shape == (22 * 7 * 7,) and len(info['rms']) == 2
    # F^ against F along phase 1: at the flown midpoints and times of the kept rows
    Xh = est['phase1']['X'].cpu().numpy()
    e = info['estimate']
    grid = WF.grid_of(e.field())
    ms = WF.measure(Xh, n_ac, 0.2, grid, rows=rows)
    err, meas = WF.recovery_error(e.cp.cpu().numpy(), grid, F, ms)
    print(f'max|F^ - F| along phase 1 = {err:.3e} m/s (largest single measurement error {meas:.3e}), rms = {info["rms"]}, '
          f'{stats["used"]:.0f} samples, {stats["cg_iters"]:.0f} CG iterations')
    assert err <= 2.0 * WF.RECOVERY_ERR['gust']
    assert float(none['wind_fit']['estimate'].cp.abs().max().item()) <= 1e-6              # the no-wind mission did plan in no wind
    for m in (true, est, none):
        assert (m['plan']['status'].cpu().numpy() == 1).all()
    e_true, e_est, e_none = (float(m['audit']['phase2']['err_max'].max().item()) for m in (true, est, none))
    print(f'phase-2 tracking error: planned in F {e_true:.4f} m, in F^ {e_est:.4f} m, in no wind {e_none:.4f} m')
    assert abs(e_est - e_true) < abs(e_none - e_true)
