"""GPU: the multi-aircraft collocation solve with every aircraft inside its scenario's convex polygon (include/d2d.h
d2d_nlp_solve_groups_fence, csrc/nlp_kernels.hip nlp_groups_body with PAIRS and FENCE) against the single-aircraft entry, against
d2d_nlp_solve_groups_pairs and against the CPU statement tests/nlp_fence_ref.solve_groups.  Tolerances against the statement: statuses
and sweeps equal, cost within 1e-7 relative, nodes 1e-4.

The coupled pair, on the CPU with the statement alone before this module was written (nlp_fence_ref.pair_scenario: legs 9 m apart inside
rcol = 10 m, the right edge `room` m on the outer side of aircraft 1): room 0.2 m settles in 3 sweeps at 17 and at 41 nodes (moved
5.4e-10 / 1.5e-8 against tol 1e-7), the edge's largest dual 0.49 / 0.20 on aircraft 1 and 2.4e-10 / 4.3e-10 on aircraft 0; room 0.5 m in
4 sweeps at both (duals 0.31 / 0.14).  0.2 m is used."""
import numpy as np
import pytest

import nlp_fence_ref as F
import nlp_groups_pairs_ref as P

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


def groups_solve(ctx, rows, W0s, n_ac, edges, h=F.H0, **kw):
    W = _dev(ctx, np.stack([w.T for w in W0s]))
    out = ctx.nlp_solve_groups_fence(_dev(ctx, rows), W, h, n_ac, None if edges is None else _dev(ctx, edges), **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in KEYS + ('sweeps', 'moved', 'fence_mult') and v is not None}
    return W.cpu().numpy().transpose(0, 2, 1), res


def test_without_masks_every_aircraft_is_the_single_entry_bit_for_bit(ctx):
    """Two scenarios of two uncoupled aircraft, each scenario with its own polygon (the full solves' corridor, and the same moved out by
    half a metre), the second aircraft from a guess moved sideways."""
    got = F.full_launch(41)[0]
    row, W0, ed = got[1], got[2], got[4]
    ed2 = ed.copy(); ed2[:4, 2] += 0.5
    rows = np.stack([row] * 4)
    W0b = W0 + np.array([0, 0.1, 0, 0, 0]); W0b[[0, -1]] = W0[[0, -1]]
    W0s = [W0, W0b, W0, W0b]
    edges = np.stack([ed, ed2])
    W, out = groups_solve(ctx, rows, W0s, 2, edges)
    Ws = _dev(ctx, np.stack([w.T for w in W0s]))
    one = ctx.nlp_solve_fence(_dev(ctx, rows), Ws, F.H0, _dev(ctx, np.repeat(edges, 2, 0)))
    ctx.sync()
    assert W.tobytes() == Ws.cpu().numpy().transpose(0, 2, 1).tobytes() and (out['status'] == 1).all() and (out['sweeps'] == 0).all()
    for k in KEYS + ('fence_mult',):
        assert out[k].tobytes() == one[k].cpu().numpy().tobytes(), k
    assert out['fence_mult'].max() > 1e-2 and not np.array_equal(W[0], W[2])


def test_with_every_edge_absent_it_is_groups_pairs_bit_for_bit(ctx):
    rows = P.pair_scenarios()[0]
    W0s = P.guesses(rows)
    for edges in (None, np.zeros((1, F.MAX_FENCE, 4))):
        W, out = groups_solve(ctx, rows, W0s, 4, edges, h=P.H, max_sweeps=3)
        Wp = _dev(ctx, np.stack([w.T for w in W0s]))
        ref = ctx.nlp_solve_groups_pairs(_dev(ctx, rows), Wp, P.H, 4, max_sweeps=3)
        ctx.sync()
        assert W.tobytes() == Wp.cpu().numpy().transpose(0, 2, 1).tobytes()
        for k in KEYS + ('sweeps', 'moved'):
            assert out[k].tobytes() == ref[k].cpu().numpy().tobytes(), k
        assert (out['sweeps'] == 3).all() and ('fence_mult' not in out or not out['fence_mult'].any())


@pytest.mark.parametrize('N', F.GROUP_N)
def test_a_coupled_pair_against_an_edge_vs_the_statement(ctx, N):
    rows, W0s, edges = F.pair_scenario(N)
    W, out = groups_solve(ctx, rows, W0s, 2, edges[None], max_sweeps=F.GROUP_SWEEPS)
    Wr, infos, sweeps, moved = F.solve_groups(rows, edges, W0s, max_sweeps=F.GROUP_SWEEPS, N=N, h=F.H0)
    k = int(np.argmin(edges[:, 1]))                              # the edge on the outer side of aircraft 1: normal (0, -1)
    for a in range(2):
        dn = float(np.abs(W[a] - Wr[a]).max())
        g = F.g_values(W[a][1:-1], edges)
        print(f'{N}-{a}: status {out["status"][a]} / {infos[a]["status"]}, steps {out["iters"][a]} / {infos[a]["inner"]}, cost {out["cost"][a]:.12f} vs '
              f'{infos[a]["cost"]:.12f}, nodes off by {dn:.2e}, min g {g.min():.2e}, edge dual {out["fence_mult"][a, k].max():.3e} / {infos[a]["zf"][k].max():.3e}')
        assert out['status'][a] == infos[a]['status'] == 1
        assert abs(out['cost'][a] - infos[a]['cost']) <= COST_RTOL * abs(infos[a]['cost']) and dn <= NODE_TOL
        assert g.min() > 0.0 and out['feas'][a] <= 1e-9
    print(f'sweeps {out["sweeps"][0]} / {sweeps}, moved {out["moved"][0]:.2e} / {moved:.2e}')
    assert out['sweeps'][0] == sweeps and 1 <= sweeps < F.GROUP_SWEEPS
    assert out['fence_mult'][1, k].max() > 1e-2 and out['fence_mult'][0, k].max() < 1e-6        # the edge binds on aircraft 1 alone


def test_a_bad_edge_or_an_end_pose_outside_refuses_its_scenario_alone(ctx):
    import d2dhip
    N = 17
    rows, W0s, edges = F.pair_scenario(N)
    bad = edges.copy(); bad[2, 3] = 0.0                          # kap = 0 on a present edge
    L = rows[1, d2dhip.SC_X1]
    out_ = edges.copy()                                          # the edge beyond the end poses pulled back to 0.1 m short of them: p1 outside
    kx = int(np.argmax(edges[:, 0])); out_[kx, 2] = L - 0.1
    tabs = np.stack([edges, bad, edges, out_])
    W, out = groups_solve(ctx, np.concatenate([rows] * 4), W0s * 4, 2, tabs, max_sweeps=F.GROUP_SWEEPS)
    print(f'status {out["status"].tolist()}, sweeps {out["sweeps"].tolist()}')
    for r in (1, 3):
        sl = slice(2 * r, 2 * r + 2)
        assert (out['status'][sl] == d2dhip.ST_NONFINITE).all() and np.isnan(out['cost'][sl]).all() and np.isnan(out['feas'][sl]).all()
        assert (out['iters'][sl] == 0).all() and out['sweeps'][r] == 0
        assert all(W[2 * r + a].tobytes() == W0s[a].tobytes() for a in range(2))
        assert F.solve_groups(rows, tabs[r], W0s, N=N, h=F.H0)[1][0]['status'] == F.ST_NONFINITE
    assert (out['status'][[0, 1, 4, 5]] == 1).all() and W[:2].tobytes() == W[4:6].tobytes() and out['sweeps'][0] == out['sweeps'][2] >= 1


def test_host_errors_and_plan_batch(ctx):
    """D2D_EINVAL before any launch, and full_sim.plan_batch(backend='nlp', fence=, n_ac=2): one GeoFence for all scenarios gives the
    direct call's bytes."""
    import d2dhip
    import d2d.opty_utils as ou
    import full_sim
    N = 17
    rows, W0s, edges = F.pair_scenario(N)
    with pytest.raises(d2dhip.D2DError, match=rf'error -1: .*n_edge = {d2dhip.MAX_FENCE + 1} outside'):
        groups_solve(ctx, rows, W0s, 2, np.zeros((1, d2dhip.MAX_FENCE + 1, 4)))
    W, out = groups_solve(ctx, rows, W0s, 2, edges[None], max_sweeps=F.GROUP_SWEEPS)
    L = 12.0 * F.H0 * (N - 1)
    gf = ou.GeoFence([(-0.5 * L, -9.2), (1.5 * L, -9.2), (1.5 * L, 5.0), (-0.5 * L, 5.0)])
    assert np.array_equal(gf.lowered(), edges)
    pl = full_sim.plan_batch(rows, N, (N - 1) * F.H0, 1.0, backend='nlp', W0=np.stack([w.T for w in W0s]), h=F.H0, n_ac=2, fence=gf,
                             max_sweeps=F.GROUP_SWEEPS)
    ctx.sync()
    assert pl['entry'] == 'nlp_solve_groups_fence' and np.array_equal(pl['W'].cpu().numpy().transpose(0, 2, 1), W)
    assert np.array_equal(pl['fence_mult'].cpu().numpy(), out['fence_mult']) and np.array_equal(pl['sweeps'].cpu().numpy(), out['sweeps'])
