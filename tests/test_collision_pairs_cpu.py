"""CPU: collision avoidance on every aircraft pair -- the host cost classes (CostCollision(pairs=), CostComposit(col_pairs=)), their
lowering to scenario rows, and the CPU statement tests/nlp_groups_pairs_ref.py: equal to nlp_groups_wind_ref with the masks of the
pair (0, 1), and the conditions its all-pairs scenarios were chosen under."""
import numpy as np
import pytest

import nlp_groups_pairs_ref as P
import nlp_groups_wind_ref as G
import nlp_wind_ref as R


class _Planner:
    """What the multi-aircraft cost plug-ins read from a planner (multi_opt_planner.Planner's free-vector layout)."""

    def __init__(self, n, N, obj_scale=1.0):
        import d2d.multiopty_utils as d2mou
        self.num_nodes, self.obj_scale, self.acs = N, obj_scale, d2mou.AircraftSet(n)
        self._slice_x = [slice((0 + 3 * i) * N, (1 + 3 * i) * N, 1) for i in range(n)]
        self._slice_y = [slice((1 + 3 * i) * N, (2 + 3 * i) * N, 1) for i in range(n)]
        self._slice_psi = [slice((2 + 3 * i) * N, (3 + 3 * i) * N, 1) for i in range(n)]
        self._slice_phi = [slice(3 * n * N + i * N, 3 * n * N + (i + 1) * N, 1) for i in range(n)]
        self._slice_v = [slice(4 * n * N + i * N, 4 * n * N + (i + 1) * N, 1) for i in range(n)]


def _free(n, N, seed=3):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1.0, 1.0, 5 * n * N)
    p = _Planner(n, N)
    for i in range(n):                          # positions a few metres apart: every pair inside the Gaussian
        f[p._slice_x[i]] = np.linspace(0.0, 20.0, N) + rng.uniform(-1, 1, N)
        f[p._slice_y[i]] = 2.5 * i + rng.uniform(-1, 1, N)
    return f, p


def test_host_cost_sums_the_selected_pairs_once():
    """a. CostCollision(pairs='all'): the cost is the sum of the single-pair costs, the gradient that of the cost (central
    differences), and pairs=None gives today's numbers exactly (the reference's expressions on aircraft 0 and 1)."""
    import d2d.multiopty_utils as d2mou
    import d2d.opty_utils as d2ou
    n, N = 4, 9
    f, p = _free(n, N)
    call = d2mou.CostCollision(r=5., pairs='all')
    single = [d2mou.CostCollision(r=5., pairs=[q]) for q in P.all_pairs(n)]
    assert call.cost(f, p) == pytest.approx(sum(c.cost(f, p) for c in single), rel=1e-14)
    np.testing.assert_allclose(call.cost_grad(f, p), sum(c.cost_grad(f, p) for c in single), rtol=1e-13, atol=1e-16)
    assert all(c.cost(f, p) > 1e-4 for c in single)
    g = call.cost_grad(f, p)
    fd = np.zeros_like(f)
    for k in range(len(f)):
        e = np.zeros_like(f); e[k] = 1e-6
        fd[k] = (call.cost(f + e, p) - call.cost(f - e, p)) / 2e-6
    # cost_grad is the reference's: -2 dx e without the chain-rule factor (k / r)^2 (oracle/nlp.py calls it the quirk)
    np.testing.assert_allclose(g * (call.k / call.r) ** 2, fd, rtol=1e-6, atol=1e-9)
    # the default: the reference's expressions, bit for bit
    c0 = d2mou.CostCollision(r=5.)
    dx, dy = f[p._slice_x[0]] - f[p._slice_x[1]], f[p._slice_y[0]] - f[p._slice_y[1]]
    e = d2ou._obstacle_field(dx, dy, 5., 1, 2.)
    assert c0.cost(f, p) == p.obj_scale / N * np.sum(e)
    g0 = np.zeros_like(f)
    g0[p._slice_x[0]], g0[p._slice_y[0]] = p.obj_scale / N * -2. * dx * e, p.obj_scale / N * -2. * dy * e
    g0[p._slice_x[1]], g0[p._slice_y[1]] = p.obj_scale / N * 2. * dx * e, p.obj_scale / N * 2. * dy * e
    assert np.array_equal(c0.cost_grad(f, p), g0)
    assert c0.cost(f, p) == pytest.approx(single[0].cost(f, p), rel=1e-15)
    # CostComposit hands the argument on
    cc = d2mou.CostComposit(kvel=70., kbank=1., kcol=10., vsp=12., rcol=5., col_pairs=[(1, 3), (0, 2)])
    ref = d2mou.CostComposit(kvel=70., kbank=1., kcol=float('nan'), vsp=12., rcol=5.)
    extra = 10. * (d2mou.CostCollision(r=5., pairs=[(1, 3)]).cost(f, p) + d2mou.CostCollision(r=5., pairs=[(0, 2)]).cost(f, p))
    assert cc.cost(f, p) == pytest.approx(ref.cost(f, p) + extra, rel=1e-14)


def _trap(cost):
    import multi_opt_planner as mop

    class S(mop.trap_4):
        pass
    S.cost = cost
    S.t1 = 6.
    S.p0s = tuple((0., -10. * i, 0., 0., 12.) for i in range(4))
    S.p1s = tuple((54., -10. * i, 0., 0., 12.) for i in range(4))
    return S


def test_lowering_writes_symmetric_partner_sets(monkeypatch):
    """b. scenario_rows and Problem._rows: masks and collision columns for 'all' and for a pair list, rows of the default byte for
    byte what the lowering wrote before `pairs` existed, ValueError for malformed pairs, more than 8 aircraft refused as before."""
    import d2dhip as D
    import d2d.multiopty_utils as d2mou
    import multi_opt_planner as mop
    import single_opt_planner as sop
    monkeypatch.setattr(sop, 'get_plan', lambda *a, **k: None)          # (the fit plan lives on the device; the rows do not)
    kw = dict(kvel=70., kbank=1., kobs=float('nan'), kcol=10., vsp=12., obss=[], obs_kind=0, rcol=10)
    S0 = _trap(d2mou.CostComposit(**kw))
    assert len(sop.lower_cost(S0.cost)) == 9 and mop.scenario_pairs(S0, 4) is None
    rows0, _, coupled0 = mop.scenario_rows(S0, S0.p0s, S0.p1s, 61, 6.0, S0.obj_scale, (0., 0.))
    # the default lowering restated: every row carries the columns, aircraft 0 and 1 the masks 0b10, 0b01
    low = sop.lower_cost(S0.cost)
    want = np.stack([sop.scen_row(p0, p1, S0.vref, low, 1.0 / 61 / 4, (0., 0.), S0.phi_constraint, S0.v_constraint,
                                  x_c=S0.x_constraint, y_c=S0.y_constraint) for p0, p1 in zip(S0.p0s, S0.p1s)])
    want[:, D.SC_KCOL], want[:, D.SC_RCOL], want[:, D.SC_SCOL] = 10., 10., 1.0 / 61
    want[0, D.SC_PMASK], want[1, D.SC_PMASK] = 2, 1
    assert coupled0 and rows0.tobytes() == want.tobytes()
    # 'all'
    Sa = _trap(d2mou.CostComposit(col_pairs='all', **kw))
    assert mop.scenario_pairs(Sa, 4) == P.all_pairs(4)
    rows, _, coupled = mop.scenario_rows(Sa, Sa.p0s, Sa.p1s, 61, 6.0, Sa.obj_scale, (0., 0.))
    assert coupled and rows[:, D.SC_PMASK].tolist() == [0b1110, 0b1101, 0b1011, 0b0111]
    assert (rows[:, D.SC_KCOL] == 10.).all() and (rows[:, D.SC_RCOL] == 10.).all() and (rows[:, D.SC_SCOL] == 1.0 / 61).all()
    other = [c for c in range(D.SCEN_STRIDE) if c not in (D.SC_PMASK, D.SC_KCOL, D.SC_RCOL, D.SC_SCOL)]
    assert np.array_equal(rows[:, other], rows0[:, other])
    # a pair list: aircraft 2 has no partner and carries neither mask nor columns
    Sl = _trap(d2mou.CostComposit(col_pairs=[(3, 1), (0, 1)], **kw))
    rows, _, coupled = mop.scenario_rows(Sl, Sl.p0s, Sl.p1s, 61, 6.0, Sl.obj_scale, (0., 0.))
    assert coupled and rows[:, D.SC_PMASK].tolist() == [0b0010, 0b1001, 0, 0b0010]
    assert rows[:, D.SC_KCOL].tolist() == [10., 10., 0., 10.] and rows[2, D.SC_RCOL] == 0. and rows[2, D.SC_SCOL] == 0.
    # the collocation Problem lowers the same sets
    pl = mop.Planner(Sl, backend='nlp')
    prow, pc = pl.prob._rows()
    assert pc and prow[:, D.SC_PMASK].tolist() == [0b0010, 0b1001, 0, 0b0010] and prow[:, D.SC_KCOL].tolist() == [10., 10., 0., 10.]
    p0 = mop.Planner(S0, backend='nlp')
    prow0, _ = p0.prob._rows()
    assert (prow0[:, D.SC_PMASK] == 0).all() and prow0[:, D.SC_KCOL].tolist() == [10., 10., 0., 0.] and p0.prob._pairs is None
    # malformed pairs: refused when the cost is lowered to rows
    for bad in ([(1, 1)], [(0, 4)], [(-1, 2)], [(0, 1), (1, 0)], [(0, 1, 2)], 'every'):
        Sb = _trap(d2mou.CostComposit(col_pairs=bad, **kw))
        with pytest.raises(ValueError):
            mop.scenario_rows(Sb, Sb.p0s, Sb.p1s, 61, 6.0, Sb.obj_scale, (0., 0.))
        with pytest.raises(ValueError):
            mop.Planner(Sb, backend='nlp').prob._rows()
    with pytest.raises(ValueError):
        d2mou.CostCollision(pairs=[(2, 2)]).cost(*_free(4, 5))
    # more than 8 aircraft: as before
    S9 = _trap(d2mou.CostComposit(col_pairs='all', **kw))
    S9.p0s = tuple((0., -10. * i, 0., 0., 12.) for i in range(9)); S9.p1s = tuple((54., -10. * i, 0., 0., 12.) for i in range(9))
    with pytest.raises(NotImplementedError):
        mop.scenario_rows(S9, S9.p0s, S9.p1s, 61, 6.0, S9.obj_scale, (0., 0.))


def test_plan_batch_routes_by_the_rows_masks():
    """The rows decide the entry point of full_sim.plan_batch: the default lowering's masks (and rows without masks) stay on
    d2d_nlp_solve_groups[_wind]; anything else goes to d2d_nlp_solve_groups_pairs."""
    import d2dhip as D
    import full_sim as fs
    rows = np.zeros((8, D.SCEN_STRIDE))
    assert not fs._rows_select_pairs(rows, 4)
    rows[0, D.SC_PMASK], rows[1, D.SC_PMASK] = 2, 1
    assert not fs._rows_select_pairs(rows, 4)
    rows[6, D.SC_PMASK], rows[7, D.SC_PMASK] = 8, 4
    assert fs._rows_select_pairs(rows, 4)
    assert fs._rows_select_pairs(np.concatenate(P.pair_scenarios()), 4) and not fs._rows_select_pairs(np.concatenate(G.group_scenarios()), 4)


def test_statement_with_the_default_pair_is_the_pair_statement():
    """c. nlp_groups_pairs_ref.solve_groups with the masks of the pair (0, 1) equals nlp_groups_wind_ref.solve_groups exactly on
    group_scenarios() (constant wind and the gust)."""
    F = R.fields()['gust']
    for r, sc in enumerate(G.group_scenarios()):
        for inner in (G.in_constant_wind(), G.in_field(F, G.T_STARTS['gust'][r])):
            Wa, ia, sa, ma = G.solve_groups(G.problems_of(sc), G.guesses(sc), inner)
            Wb, ib, sb, mb = P.solve_groups(P.problems_of(sc), P.guesses(sc), inner, [0b10, 0b01, 0, 0])
            assert sa == sb and ma == mb
            for a in range(4):
                assert np.array_equal(Wa[a], Wb[a])
                assert all(ia[a][k] == ib[a][k] for k in ('status', 'inner', 'cost', 'feas'))


def _solve(rows, wind, r, W0s=None, max_sweeps=P.MAX_SWEEPS):
    inner = P.in_constant_wind() if wind == 'const' else P.in_field(R.fields()[wind], P.T_STARTS[wind][r])
    return P.solve_groups(P.problems_of(rows), P.guesses(rows) if W0s is None else W0s, inner, P.masks_of(rows), max_sweeps=max_sweeps)


@pytest.mark.parametrize('wind', ['const', 'shear', 'vortex', 'gust'])
def test_all_pairs_scenarios_meet_the_conditions_they_were_chosen_under(wind):
    """d. Every all-pairs scenario, in the constant wind and in the three fields: every inner solve converges, the group settles at
    tol 1e-7 with at least two sweeps to spare under MAX_SWEEPS, and under a 1e-9 perturbation of the guesses the sweep count does
    not change.  Uncoupled, three different pairs come inside rcol in the scenarios' own constant wind (in a field at least two, both
    other than (0, 1): the fields move the tracks)."""
    rng = np.random.default_rng(1)
    for r, rows in enumerate(P.pair_scenarios()):
        Ws, infos, sweeps, moved = _solve(rows, wind, r)
        assert all(i['status'] == 1 for i in infos) and moved <= 1e-7 and 1 <= sweeps <= P.MAX_SWEEPS - 2, (r, sweeps, moved)
        Wp, ip, sp, mp = _solve(rows, wind, r, [w + 1e-9 * rng.standard_normal(w.shape) for w in P.guesses(rows)])
        assert sp == sweeps and all(i['status'] == 1 for i in ip)
        import d2dhip as D
        unc = rows.copy(); unc[:, D.SC_PMASK] = 0
        Wu, iu, su, _ = _solve(unc, wind, r)
        near = [p for p, d in P.min_separation(Wu, P.all_pairs(4)).items() if d < P.RCOL]
        print(wind, r, 'sweeps', sweeps, 'moved %.1e' % moved, 'inside rcol uncoupled', near)
        assert su == 0 and len(near) >= (3 if wind == 'const' else 2) and sum(p != (0, 1) for p in near) >= 2


def test_all_pairs_keep_the_other_pairs_further_apart_on_the_cpu():
    """The ordering the GPU effect test asserts, on the CPU first (constant wind): every pair other than (0, 1) that the default
    pair leaves inside rcol is further apart under 'all'."""
    for r, (rows, rows01) in enumerate(zip(P.pair_scenarios(), P.pair_scenarios([(0, 1)]))):
        Wa, ia, _, _ = _solve(rows, 'const', r)
        Wd, idf, _, _ = _solve(rows01, 'const', r)
        sa, sd = P.min_separation(Wa, P.all_pairs(4)), P.min_separation(Wd, P.all_pairs(4))
        near = [p for p in P.all_pairs(4) if p != (0, 1) and sd[p] < P.RCOL]
        print(r, {p: (round(sd[p], 3), round(sa[p], 3)) for p in near})
        assert len(near) >= 2 and all(sa[p] > sd[p] for p in near)
