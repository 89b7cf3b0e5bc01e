"""GPU: the multi-aircraft collocation solve with every aircraft outside its scenario's hard moving discs (include/d2d.h
d2d_nlp_solve_groups_keepout, csrc/nlp_kernels.hip nlp_groups_body with PAIRS and KMOV) against the single-aircraft entry, against
d2d_nlp_solve_groups_pairs and against the CPU statement tests/nlp_keepout_moving_ref.solve_groups.  Tolerances against the statement:
those of tests/test_gpu_moving_obstacles.py -- statuses and sweeps equal, cost within 1e-7 relative (of max(cost, 1e-3)), nodes 1e-4."""
import numpy as np
import pytest

import nlp_groups_pairs_ref as P
import nlp_keepout_moving_ref as KM
import nlp_keepout_ref as K

pytestmark = pytest.mark.gpu
COST_RTOL, NODE_TOL = 1e-7, 1e-4
KEYS = ('cost', 'feas', 'iters', 'status')


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    return ctx.dev(np.ascontiguousarray(a))


def groups_solve(ctx, rows, W0s, n_ac, knots, disc, t_start, **kw):
    W = _dev(ctx, np.stack([w.T for w in W0s]))
    out = ctx.nlp_solve_groups_keepout(_dev(ctx, rows), W, K.H0, n_ac, _dev(ctx, knots), _dev(ctx, disc), t_start=t_start, **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in KEYS + ('sweeps', 'moved', 'keep_mult') and v is not None}
    return W.cpu().numpy().transpose(0, 2, 1), res


def test_without_masks_every_aircraft_is_the_single_entry_bit_for_bit(ctx):
    """Two scenarios of two uncoupled aircraft (the full solves' leg twice, each scenario with its own disc)."""
    got = KM.full_launch(41)
    rows = np.stack([got[0][1], got[0][1], got[1][1], got[1][1]])
    W0s = [got[0][2], got[0][2] * np.array([1, 1.0, 1, 1, 1]) + np.array([0, 0.3, 0, 0, 0]), got[1][2], got[1][2]]
    W0s[1][[0, -1]] = got[0][2][[0, -1]]
    knots, disc = KM.tables([got[0][3], got[1][3]])
    W, out = groups_solve(ctx, rows, W0s, 2, knots, disc, KM.FULL_T_START)
    Ws = _dev(ctx, np.stack([w.T for w in W0s]))
    one = ctx.nlp_solve_keepout_moving(_dev(ctx, rows), Ws, K.H0, _dev(ctx, np.repeat(knots, 2, 0)), _dev(ctx, np.repeat(disc, 2, 0)), t_start=KM.FULL_T_START)
    ctx.sync()
    assert W.tobytes() == Ws.cpu().numpy().transpose(0, 2, 1).tobytes() and (out['status'] == 1).all() and (out['sweeps'] == 0).all()
    for k in KEYS + ('keep_mult',):
        assert out[k].tobytes() == one[k].cpu().numpy().tobytes(), k
    assert out['keep_mult'].any()


def test_with_every_radius_absent_it_is_groups_pairs_bit_for_bit(ctx):
    rows = P.pair_scenarios()[0]
    W0s = P.guesses(rows)
    trs = [KM.line_track((0.0, 0.0), (1.0, 2.0), 3.0, 6.0, 0.0), KM.line_track((5.0, 0.0), (-1.0, 2.0), 3.0, 6.0, -1.0)]
    knots, disc = KM.tables([trs])
    W, out = groups_solve(ctx, rows, W0s, 4, knots, disc, 0.5, max_sweeps=3)
    Wp = _dev(ctx, np.stack([w.T for w in W0s]))
    ref = ctx.nlp_solve_groups_pairs(_dev(ctx, rows), Wp, P.H, 4, max_sweeps=3)
    ctx.sync()
    assert W.tobytes() == Wp.cpu().numpy().transpose(0, 2, 1).tobytes()
    for k in KEYS + ('sweeps', 'moved'):
        assert out[k].tobytes() == ref[k].cpu().numpy().tobytes(), k
    assert not out['keep_mult'].any() and (out['sweeps'] == 3).all()


@pytest.mark.parametrize('N', KM.GROUP_N)
def test_a_coupled_pair_round_a_crossing_disc_vs_the_statement(ctx, N):
    rows, W0s, trs = KM.pair_scenario(N)
    knots, disc = KM.tables([trs])
    W, out = groups_solve(ctx, rows, W0s, 2, knots, disc, KM.GROUP_T_START, max_sweeps=KM.GROUP_SWEEPS)
    Wr, infos, sweeps, moved = KM.solve_groups(rows, trs, W0s, t_start=KM.GROUP_T_START, max_sweeps=KM.GROUP_SWEEPS, N=N, h=K.H0)
    ctr, R = KM.centres(trs, KM.GROUP_T_START, N, K.H0)
    for a in range(2):
        dn = float(np.abs(W[a] - Wr[a]).max())
        g = KM.g_values(W[a][1:-1], ctr[:, 1:-1], R)[0]
        print(f'{N}-{a}: status {out["status"][a]} / {infos[a]["status"]}, steps {out["iters"][a]} / {infos[a]["inner"]}, cost {out["cost"][a]:.12f} vs '
              f'{infos[a]["cost"]:.12f}, nodes off by {dn:.2e}, min g {g.min():.2e}, z max {out["keep_mult"][a].max():.3e}')
        assert out['status'][a] == infos[a]['status'] == 1
        assert abs(out['cost'][a] - infos[a]['cost']) <= COST_RTOL * max(infos[a]['cost'], 1e-3) and dn <= NODE_TOL
        assert g.min() > 0.0 and out['feas'][a] <= 1e-9
    print(f'sweeps {out["sweeps"][0]} / {sweeps}, moved {out["moved"][0]:.2e} / {moved:.2e}')
    assert out['sweeps'][0] == sweeps and 1 <= sweeps < KM.GROUP_SWEEPS
    assert out['keep_mult'][0, 0].max() > 1e-2 and out['keep_mult'][1, 0].max() < 1e-6       # the disc binds on aircraft 0 alone


def test_a_bad_track_refuses_its_scenario_alone(ctx):
    import d2dhip
    N = 17
    rows, W0s, trs = KM.pair_scenario(N)
    knots, disc = KM.tables([trs] * 3)
    knots[1, 0, 1, 2] = np.inf
    W, out = groups_solve(ctx, np.concatenate([rows] * 3), W0s * 3, 2, knots, disc, KM.GROUP_T_START, max_sweeps=KM.GROUP_SWEEPS)
    print(f'status {out["status"].tolist()}, sweeps {out["sweeps"].tolist()}')
    assert (out['status'][2:4] == d2dhip.ST_NONFINITE).all() and np.isnan(out['cost'][2:4]).all() and np.isnan(out['feas'][2:4]).all()
    assert (out['iters'][2:4] == 0).all() and out['sweeps'][1] == 0
    assert all(W[2 + a].tobytes() == W0s[a].tobytes() for a in range(2))
    assert (out['status'][[0, 1, 4, 5]] == 1).all() and W[:2].tobytes() == W[4:].tobytes() and out['sweeps'][0] == out['sweeps'][2] >= 1
    # an aircraft whose end pose lies inside the disc at node N - 1's time refuses its scenario too
    L = rows[1, d2dhip.SC_X1]
    T = (N - 1) * K.H0
    arrive = KM.Track((KM.GROUP_T_START, KM.GROUP_T_START + T), ((L, -40.0), (L, -9.0 + 0.3)), trs[0].r)
    knots, disc = KM.tables([trs, [arrive]])
    W, out = groups_solve(ctx, np.concatenate([rows] * 2), W0s * 2, 2, knots, disc, KM.GROUP_T_START, max_sweeps=KM.GROUP_SWEEPS)
    assert (out['status'][:2] == 1).all() and (out['status'][2:] == d2dhip.ST_NONFINITE).all() and out['sweeps'][1] == 0
    assert all(W[2 + a].tobytes() == W0s[a].tobytes() for a in range(2))
    assert KM.solve_groups(rows, [arrive], W0s, t_start=KM.GROUP_T_START, N=N, h=K.H0)[1][0]['status'] == KM.ST_NONFINITE
