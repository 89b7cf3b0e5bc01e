"""CPU: the statement of the collocation solve inside a convex polygon (tests/nlp_fence_ref.py) against the SLSQP arbiter, its pieces
against finite differences, d2d.opty_utils.GeoFence, the convexity guarantee, the host routes' refusals, the header and the binding.
No device is touched."""
import os
import re

import numpy as np
import pytest

import nlp_fence_ref as F
import nlp_keepout_ref as K
import nlp_steps_ref as S
from oracle import nlp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'nlp_fence_slsqp.npz')
# ten times the statement's largest relative cost difference to SLSQP over the golden cases, 8.34e-9 (tests/golden/make_nlp_fence_golden.py
# prints it)
SLSQP_COST_RTOL = 8.4e-8


def test_no_edges_is_the_keepout_statement_bit_for_bit():
    for N, two in ((9, False), (17, True)):
        pb, row, W0, discs = K.arbiter_problem(N, two)
        Wk, ik = K.solve(K.Plain(pb), W0, discs)
        for edges in (np.zeros((0, 4)), np.zeros((F.MAX_FENCE, 4))):
            Wf, info = F.solve(F.Plain(pb), W0, discs, edges)
            assert np.array_equal(Wf, Wk) and info['cost'] == ik['cost'] and info['inner'] == ik['inner'] and info['status'] == ik['status']
            assert np.array_equal(info['zk'], ik['zk']) and np.array_equal(info['mult'], ik['mult']) and info['zf'].shape == (len(edges), N)
    pb, row, W0, _ = K.arbiter_problem(9, False)
    Wo, io = nlp.solve(pb, W0)
    Wf, info = F.solve(F.Plain(pb), W0, np.zeros((0, 3)), np.zeros((0, 4)))
    assert np.array_equal(Wf, Wo) and info['cost'] == io['cost'] and info['inner'] == io['inner']


def test_barrier_gradient_and_block_match_central_differences():
    """rhs (with mub / g) is minus the gradient of - mub sum log g; with z = mub / g the 2x2 block (doubled: half convention) is its
    Hessian; the stationarity term is the gradient of - sum z g at fixed z."""
    pb, row, W0, discs, edges = F.arbiter_problem('roof-9')
    W = F.start(pb, W0, discs, edges)
    mub = 0.03
    g = F.g_values(W[1:-1], edges)
    assert (g > 0).all()
    zf = mub / g
    rhs, st, blk = F.barrier_terms(W, edges, zf, mub)
    eps = 1e-6
    for i in (1, 4, 7):
        grad = np.zeros(2)
        for c in range(2):
            Wp, Wm = W.copy(), W.copy()
            Wp[i, c] += eps; Wm[i, c] -= eps
            grad[c] = (F.barrier_value(Wp, edges, mub) - F.barrier_value(Wm, edges, mub)) / (2 * eps)
            gp = np.zeros(2)
            for d in range(2):
                e2 = 1e-4                                # (second differences: 1e-16 / e2^2 of rounding against (e2 / g)^2 of truncation, g ~ 0.1)
                Ws = [W.copy() for _ in range(4)]
                for Wq, (sc, sd) in zip(Ws, ((1, 1), (1, -1), (-1, 1), (-1, -1))):
                    Wq[i, c] += sc * e2; Wq[i, d] += sd * e2
                v = [F.barrier_value(Wq, edges, mub) for Wq in Ws]
                gp[d] = (v[0] - v[1] - v[2] + v[3]) / (4 * e2 * e2)
            assert np.allclose(2.0 * blk[i, c], gp, rtol=1e-4, atol=1e-5 * np.abs(blk[i]).max())
        assert np.allclose(-rhs[i], grad, rtol=1e-6, atol=1e-9)
        assert np.allclose(st[i], -rhs[i])                 # z = mub / g: on the central path the two agree
    assert not rhs[[0, -1]].any() and not blk[[0, -1]].any()


def test_ratio_test_is_exact():
    """a = tau g / (a.s): g at W + a s is (1 - tau) g at the edge that binds, and larger at every other."""
    rng = np.random.default_rng(5)
    pb, row, W0, discs, edges = F.arbiter_problem('roof-9')
    W = F.start(pb, W0, discs, edges)
    for _ in range(50):
        s = rng.standard_normal((pb.N - 2, 2))
        g = F.g_values(W[1:-1], edges)
        as_ = edges[:, 0, None] * s[:, 0] + edges[:, 1, None] * s[:, 1]
        tau = 0.99
        with np.errstate(divide='ignore'):
            a = np.where(as_ > 0, tau * g / as_, np.inf).min()
        Wn = W.copy(); Wn[1:-1, :2] += a * s
        ratio = F.g_values(Wn[1:-1], edges) / g
        assert abs(ratio.min() - (1.0 - tau)) <= 1e-12 and (ratio > 0).all()


def test_geofence_validation_and_lowering():
    import d2d.opty_utils as ou
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, -s], [s, c]])
    V = np.array([[-2.0, -1.0], [2.0, -1.0], [2.0, 1.0], [-2.0, 1.0]]) @ rot.T + (5.0, 3.0)
    m = 0.1
    f = ou.GeoFence(V, m)
    rows = f.lowered()
    ctr = np.array([5.0, 3.0])
    # the four expected rows: normals -ey, +ex, +ey, -ex rotated; b = a . centre + half width; kap = 1e-2 of the shrunk width along a
    exp = []
    for a0, half, width in (((0.0, -1.0), 1.0, 2.0), ((1.0, 0.0), 2.0, 4.0), ((0.0, 1.0), 1.0, 2.0), ((-1.0, 0.0), 2.0, 4.0)):
        a = rot @ np.array(a0)
        exp.append((a[0], a[1], float(a @ ctr) + half - m, 1e-2 * (width - 2 * m)))
    assert np.allclose(rows, np.array(exp), rtol=0, atol=1e-12)
    assert np.abs(np.hypot(rows[:, 0], rows[:, 1]) - 1.0).max() <= 1e-15
    # orientation does not matter: the same set of rows from the clockwise list
    rcw = ou.GeoFence(V[::-1], m).lowered()
    assert sorted(map(tuple, np.round(rcw, 12))) == sorted(map(tuple, np.round(rows, 12)))
    assert np.array_equal(ou.lower_fence(f), rows) and np.array_equal(ou.lower_fence(rows), rows)
    # clearance is against the user's polygon
    assert np.allclose(ou.fence_clearance(f, [5.0], [3.0]), [1.0, 2.0, 1.0, 2.0])
    assert np.allclose(ou.fence_clearance(rows, [5.0], [3.0]), [0.9, 1.9, 0.9, 1.9])            # lowered rows: their own half-planes
    assert ou.fence_clearance(np.r_[rows, np.zeros((1, 4))], [5.0], [3.0])[4] == np.inf
    for bad, word in (([[0, 0], [1, 0], [1, 0], [0, 1]], 'vertex 2 repeats vertex 1'), ([[0, 0], [1, 0], [2, 0], [0, 1]], 'vertex 1 is collinear'),
                      ([[0, 0], [2, 0], [1, 0.2], [2, 2], [0, 2]], 'not convex at vertex 2'), ([[0, 0], [1, 0]], '3 to 8'),
                      (np.stack([np.cos(np.arange(9.0)), np.sin(np.arange(9.0))], 1), '3 to 8'), ([[0, 0], [1, 0], [np.nan, 1]], 'finite')):
        with pytest.raises(ValueError, match=word):
            ou.GeoFence(bad)
    star = np.arange(5) * 4 * np.pi / 5
    with pytest.raises(ValueError, match='crosses itself'):
        ou.GeoFence(np.stack([np.cos(star), np.sin(star)], 1))
    for mm in (-0.1, np.nan):
        with pytest.raises(ValueError, match='margin >= 0'):
            ou.GeoFence(V, mm)
    with pytest.raises(ValueError, match='leaves nothing'):
        ou.GeoFence(V, 1.0)
    assert len(ou.GeoFence(np.stack([np.cos(np.arange(8) * np.pi / 4), np.sin(np.arange(8) * np.pi / 4)], 1)).lowered()) == 8
    with pytest.raises(ValueError, match='rows'):
        ou.lower_fence(np.zeros((3, 3)))


def test_convexity_guarantee_on_random_segments():
    """400 segments with both ends inside the lowered fence: every point of each keeps the margin to the user's polygon."""
    import d2d.opty_utils as ou
    rng = np.random.default_rng(11)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 7))
    f = ou.GeoFence(np.stack([10 * np.cos(ang), 6 * np.sin(ang)], 1) + (3.0, -2.0), margin=0.4)
    rows = f.lowered()
    n = 0
    while n < 400:
        p, q = rng.uniform(-12, 12, 2) + (3.0, -2.0), rng.uniform(-12, 12, 2) + (3.0, -2.0)
        if F.g_values(np.array([p, q]), rows).min() <= 0.0:
            continue
        n += 1
        t = np.linspace(0.0, 1.0, 101)[:, None]
        pts = p + t * (q - p)
        assert min(ou.fence_clearance(f, pts[:, 0], pts[:, 1])) >= f.margin - 1e-12
        assert F.g_values(pts, rows).min() >= F.segment_inside(rows, p, q) - 1e-12 > -1e-12


def test_start_rule_and_refusals():
    pb, row, W0, discs, edges = F.arbiter_problem('cut-17')
    prob = F.Plain(pb)
    p0, ax, nrm, ll = F.leg_frame(pb)
    # a guess with g >= kap everywhere is not touched, bit for bit
    assert (F.g_values(W0[1:-1], edges) >= edges[:, 3, None]).all()
    assert np.array_equal(F.start(pb, W0, discs, edges), W0)
    # a node outside moves along the inward normal to g = kap; the others stay
    W = W0.copy(); W[8, :2] += 3.0 * nrm
    Ws = F.start(pb, W, discs, edges)
    k = int(np.argmax(edges[:, :2] @ nrm))
    assert abs(F.g_values(Ws[8:9], edges)[k, 0] - edges[k, 3]) <= 1e-12 and abs((Ws[8, :2] - W[8, :2]) @ ax) <= 1e-12
    assert np.array_equal(np.delete(Ws, 8, 0), np.delete(W, 8, 0)) and np.array_equal(Ws[:, 2:], W[:, 2:])
    # at a corner the second pass undoes a push off one edge into its neighbour's margin
    tri = F.fence_rows(np.array([p0 - 0.5 * ll * ax - ll * nrm, p0 + 1.5 * ll * ax - ll * nrm, p0 + 0.5 * ll * ax + 0.2 * ll * nrm]))
    W = W0.copy(); W[8, :2] = p0 + 0.5 * ll * ax + 0.25 * ll * nrm - 0.02 * ll * ax
    Ws = F.start(pb, W, discs, tri)
    assert (F.g_values(Ws[1:-1], tri) > 0).all()
    for bad, why in ((np.r_[edges, [[0.0, 0.0, np.nan, 0.0]]], 'non-finite'), (edges * (1 + 1e-9, 1 + 1e-9, 1, 1), '|a|'),
                     (edges * (1, 1, 1, 0), 'kap'), (edges * (1, 1, 1, -1), 'kap'),
                     (np.r_[edges, [[ax[0], ax[1], float(ax @ pb.p1[:2]), 0.1]]], 'p1 on an edge'),
                     (np.r_[edges, [[nrm[0], nrm[1], float(nrm @ p0) + 5e-4, 1.0], [-nrm[0], -nrm[1], -float(nrm @ p0) + 5e-4, 1.0]]], 'no room')):
        Wr, info = F.solve(prob, W0, discs, bad)
        assert info['status'] == F.ST_NONFINITE and np.isnan(info['cost']) and np.isnan(info['feas']) and np.array_equal(Wr, W0) and info['inner'] == 0, why
    # an edge with |a| off by 1e-13 is accepted
    assert F.solve(prob, W0, discs, edges * (1 + 1e-13, 1 + 1e-13, 1, 1), inner_max=1, outer_max=1)[1]['status'] != F.ST_NONFINITE


def golden_cases():
    g = np.load(GOLDEN)
    assert int(g['n_cases']) == len(F.ARB_CASES)
    for k, name in enumerate(F.ARB_CASES):
        N = int(g[f'c{k}_N'])
        yield name, nlp.problem_from_row(g[f'c{k}_row'], N, F.H0), g[f'c{k}_W0'], g[f'c{k}_discs'], g[f'c{k}_edges'], float(g[f'c{k}_cost'])


def test_statement_vs_slsqp_golden():
    worst = 0.0
    for name, pb, W0, discs, edges, cost in golden_cases():
        _, _, W0r, dr, er = F.arbiter_problem(name)
        assert np.array_equal(W0, W0r) and np.array_equal(discs, dr) and np.array_equal(edges, er)       # the file is the generator's
        W, info = F.solve(F.Plain(pb), W0, discs, edges)
        dc = abs(info['cost'] - cost) / cost
        worst = max(worst, dc)
        g = F.g_values(W[1:-1], edges)
        zmax = info['zf'].max(1)
        print(f'{name}: status {info["status"]}, {info["inner"]} steps, cost off by {dc:.2e} relative, min g {g.min():.1e}, edge duals {np.array2string(zmax, precision=3)}')
        assert info['status'] == 1 and info['feas'] <= 1e-9 and (g > 0).all()
        assert g.min() < 1e-6 and zmax.max() > 1e-3         # an edge binds: the case tests the constraint
        assert dc <= SLSQP_COST_RTOL
        if name.startswith('roof'):
            assert (zmax > 1e-3).sum() == 2
        if name.startswith('mixed'):
            assert info['zk'].max() > 1e-3 and (K.g_values(W[1:-1], discs)[0] > 0).all()
    print(f'largest: {worst:.2e}')


def test_full_solves_hold_the_margin():
    """... and are determined: the statement takes the same number of steps from 8 starts in which every entry moves by -1, 0 or +1 ulp
    (the GPU test asks the kernel for that number)."""
    import zlib
    import d2d.opty_utils as ou
    for N in F.FULL_N:
        for b, (prob, r, W0, dk, ed, gf) in enumerate(F.full_launch(N)):
            W, info = F.solve(prob, W0, dk, ed)
            act = ed[F.present(ed)]
            g = F.g_values(W[1:-1], act)
            zf = info['zf'][:len(act), 1:-1]
            assert info['status'] == 1 and info['feas'] <= 1e-9 and (g > 0).all()
            assert zf.max() > 1e-2 and np.abs(zf * g - nlp.MUB_MIN).max() <= 1e-7
            assert b == 0 or info['zk'].max() > 1e-2
            assert min(ou.fence_clearance(gf, W[:, 0], W[:, 1])) >= gf.margin
            rng = np.random.default_rng(zlib.crc32(f'full-{N}-{b}'.encode()))
            for _ in range(8):
                sgn = rng.integers(-1, 2, W0.shape)
                Wp = np.where(sgn > 0, np.nextafter(W0, np.inf), np.where(sgn < 0, np.nextafter(W0, -np.inf), W0))
                assert F.solve(prob, Wp, dk, ed)[1]['inner'] == info['inner'], (N, b)
            Wfree = F.free_plan(N)[3]
            assert min(ou.fence_clearance(gf, Wfree[:, 0], Wfree[:, 1])) < 0.0 < gf.margin          # the free plan leaves the polygon


@pytest.mark.parametrize('N', F.STEP_N)
def test_step_cases_are_determined(N):
    """Every case of the GPU step comparison, on the statement alone (nlp_steps_ref.check): its tolerance is at most 1e-8 and the
    perturbed starts take the same path after every budget; budgets with outer_max = 1 end at 'max iterations' with every step
    accepted and moving W by 1e6 tolerances.  At 3 and 5 nodes the first inner problem is solved within 8 steps, so there the budget
    (8, 1) is held to the first two checks only (as in tests/test_nlp_keepout_cpu.py).  The edges act in every case: the start rule moves
    nodes of the bowed start, and after the last budget the left edge's largest dual is above mub / (STEP_EDGE L) -- on the central path,
    z = mub / g, a node is closer to the edge than the leg's axis is."""
    for tag, (case, r, discs, edges, prob) in F.steps_launch(N).items():
        pb = prob.pb
        for budget in S.BUDGETS:
            bad = S.check(case, budget)
            if N <= 5 and budget == (8, 1):
                bad = [b for b in bad if b.startswith('tol') or b.startswith('the perturbed')]
            assert not bad, (case.cid, budget, bad)
        W0 = case.W0[0][:N]
        assert not np.array_equal(F.start(pb, W0, discs, edges)[1:-1, :2], W0[1:-1, :2])
        raw = S.measure(case, S.BUDGETS[-1])['info']['raw']
        L = 11.5 * F.H0 * (N - 1)
        room = F.STEP_EDGE * L if tag != 'disc' else (1.3 * F.STEP_DISC + 0.03) * L
        assert raw['zf'].max() > raw['mub'] / room, (case.cid, raw['zf'].max(), raw['mub'] / room)
        if tag == 'many':
            assert not F.present(edges)[[2, 5]].any() and F.present(edges).sum() == F.MAX_FENCE - 2
            assert not raw['zf'][[2, 5]].any()
        if tag == 'disc':
            assert (discs[:, 2] > 0).sum() == 1 and raw['zk'].max() > 0.0


def test_nlp_plan_routes_and_refuses_by_name():
    import d2dhip

    class _Stub:
        def nlp_solve_fence(self, scen, W, h, edges, **kw):
            return dict(args=(scen, W, h, edges), kw=kw)
    out = d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, fence='E', keep='K', field='F', t_start=2.0, inner_max=7)
    assert out['entry'] == 'nlp_solve_fence' and out['args'] == ('S', 'W', 0.1, 'E')
    assert out['kw'] == dict(discs='K', field='F', t_start=2.0, inner_max=7)
    assert d2dhip.nlp_plan(_Stub(), 'S', 'W', 0.1, fence='E')['kw']['discs'] is None
    with pytest.raises(NotImplementedError, match='fence together with keep and n_ac'):
        d2dhip.nlp_plan(None, None, None, 0.1, fence='E', keep='K', n_ac=2)

    class _GStub:
        def nlp_solve_groups_fence(self, scen, W, h, n_ac, edges, **kw):
            return dict(args=(scen, W, h, n_ac, edges), kw=kw)
    out = d2dhip.nlp_plan(_GStub(), 'S', 'W', 0.1, fence='E', n_ac=3, field='F', t_start=2.0, max_sweeps=5)
    assert out['entry'] == 'nlp_solve_groups_fence' and out['args'] == ('S', 'W', 0.1, 3, 'E') and out['kw'] == dict(field='F', t_start=2.0, max_sweeps=5)
    for kw, name in ((dict(free_rows='x'), 'free_rows'), (dict(via='x'), 'via'), (dict(knots='x'), 'knots'),
                     (dict(disc='x'), 'disc'), (dict(hard_knots='x', hard_disc='y'), 'hard_knots')):
        with pytest.raises(NotImplementedError, match=f'fence together with {name}'):
            d2dhip.nlp_plan(None, None, None, 0.1, fence='E', **kw)


def test_header_version_and_binding():
    import d2dhip
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 127
    assert 'd2d_nlp_solve_fence' in hdr and 'd2d_fence' in hdr
    assert int(re.search(r'#define D2D_MAX_FENCE (\d+)', hdr).group(1)) == d2dhip.MAX_FENCE == F.MAX_FENCE
    assert 'd2d_nlp_solve_fence' in d2dhip.EXPORTS and 'd2d_nlp_solve_groups_fence' in d2dhip.EXPORTS and 'd2d_nlp_solve_groups_fence' in hdr
    assert [n for n, _ in d2dhip.FenceC._fields_] == ['n_edge', 'pad', 'edges']


def test_plan_batch_and_the_mission_chain_refuse_by_name():
    """What the fence does not go with, each refused by name before a context is made or anything is launched."""
    import d2d.opty_utils as ou
    import full_sim
    gf = F.full_launch(17)[0][5]
    rows = np.zeros((2, 4))                      # (place holders: every refusal comes before the rows are read)
    with pytest.raises(NotImplementedError, match='polynomial fit has no geofence'):
        full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, backend='fit', fence=gf)
    mk = ou.MovingKeepOut.linear((0.0, 0.0), (1.0, 0.0), 1.0)
    with pytest.raises(NotImplementedError, match='keep_out with n_ac > 1 is not supported'):      # keep_out in the group route
        full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, backend='nlp', W0=np.zeros((2, 5, 17)), h=0.1, fence=gf, n_ac=2, keep_out=np.zeros((2, 1, 3)))
    for kw, name in ((dict(moving=[ou.MovingObstacle((0.0, 1.0), ((0.0, 0.0), (1.0, 0.0)), 1.0)]), 'moving'),
                     (dict(via=[[], []]), 'via'), (dict(free_time=(0.05, 0.2)), 'free_time'), (dict(hard_moving=[mk]), 'hard_moving'),
                     (dict(deconflict=dict(d_sep=4.0, margin=1.0, d_look=50.0)), 'deconflict')):
        with pytest.raises(NotImplementedError, match=f'fence with {name} is not supported'):
            full_sim.plan_batch(rows, 17, 1.6, 1.0 / 17, backend='nlp', W0=np.zeros((2, 5, 17)), h=0.1, fence=gf, **kw)
    with pytest.raises(NotImplementedError, match='mission chain has no geofence'):
        full_sim.full_sim_phases_batch(None, None, None, 2, None, type('m', (), dict(fence=gf)), None, 10.0)


@pytest.mark.parametrize('N', F.GROUP_N)
def test_the_coupled_pair_settles_on_the_statement(N):
    """The scenario of tests/test_gpu_groups_fence.py on the CPU alone: the alternation settles well inside max_sweeps, the edge on the
    outer side of aircraft 1 binds on aircraft 1 and not on aircraft 0."""
    rows, W0s, edges = F.pair_scenario(N)
    Ws, infos, sweeps, moved = F.solve_groups(rows, edges, W0s, max_sweeps=F.GROUP_SWEEPS, N=N, h=F.H0)
    k = int(np.argmin(edges[:, 1]))
    print(f'{N}: sweeps {sweeps}, moved {moved:.1e}, duals {infos[0]["zf"][k].max():.2e} / {infos[1]["zf"][k].max():.2e}')
    assert [i['status'] for i in infos] == [1, 1] and 1 <= sweeps < F.GROUP_SWEEPS and moved <= 1e-7
    assert infos[1]['zf'][k].max() > 1e-2 and infos[0]['zf'][k].max() < 1e-6
    assert all((F.g_values(W[1:-1], edges) > 0).all() for W in Ws)
    # no edges: nlp_groups_pairs_ref.solve_groups on the same inner solves
    assert F.solve_groups(rows, np.zeros((0, 4)), W0s, max_sweeps=2, N=N, h=F.H0)[2] >= 1


# ---- the planners: construction and refusals, no device (the runs are in tests/test_gpu_nlp_fence.py, as the neighbours' are) -------------
def _exp14(**attrs):
    import d2d.optyplan_scenarios as sc
    return type('exp_14_f', (sc.exp_14,), attrs)


def scenario_fence(e, left, right, margin=0.0):
    """A GeoFence round a single-aircraft scenario's leg: `left` / `right` of its axis, half a leg behind p0 and beyond p1."""
    import d2d.opty_utils as ou
    p0, p1 = np.array(e.p0[:2], float), np.array(e.p1[:2], float)
    ll = float(np.hypot(*(p1 - p0))); ax = (p1 - p0) / ll; nrm = np.array([-ax[1], ax[0]])
    return ou.GeoFence([p0 - 0.5 * ll * ax - right * nrm, p1 + 0.5 * ll * ax - right * nrm, p1 + 0.5 * ll * ax + left * nrm, p0 - 0.5 * ll * ax + left * nrm], margin)


def test_planner_routes_a_scenario_with_a_fence_and_refuses_by_name():
    import d2d.optyplan_scenarios as sc
    import d2d.multioptyplan_scenarios as msc
    import d2d.opty_utils as ou
    import multi_opt_planner as mop
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    gf = scenario_fence(sc.exp_14, 50.0, 50.0, 1.0)
    # 'auto' goes straight to the collocation backend; the rows are the lowering; with and without keep_out
    for kw in ({}, dict(keep_out=[ou.KeepOut((2.88, -4.54), 5.0, margin=1.0)])):
        p = sop.Planner(_exp14(fence=gf, **kw), backend='auto')
        assert isinstance(p.prob, odc.Problem) and p.prob.fence is gf and np.array_equal(p.prob.fence_rows, gf.lowered()) and p.fence is gf
    q = sop.Planner(_exp14())
    assert isinstance(q.prob, sop._FitProblem) and q.fence is None                    # without it: as before
    with pytest.raises(NotImplementedError, match="backend='fit' cannot hold a geofence"):
        sop.Planner(_exp14(fence=gf), backend='fit')
    t0, t1 = sc.exp_14.t0, sc.exp_14.t1
    for attrs, name in ((dict(moving_obstacles=[ou.MovingObstacle.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), 'moving obstacles'),
                        (dict(waypoints=[ou.Waypoint(t0 + 1.0, x=1.0)]), 'waypoints'), (dict(t1_free=(t1 - 1.0, t1 + 1.0)), 'a free duration'),
                        (dict(keep_out=[ou.MovingKeepOut.linear((90.0, 0.0), (0.0, 5.0), 4.0)]), 'a MovingKeepOut')):
        with pytest.raises(NotImplementedError, match=f'fence together with {name}'):
            sop.Planner(_exp14(fence=gf, **attrs), backend='nlp')

    class Odd:                                   # a cost plug-in no kernel knows: the host objective
        def cost(self, free, planner):
            return float(np.sum(free ** 2))

        def cost_grad(self, free, planner):
            return 2.0 * free
    with pytest.raises(NotImplementedError, match='fence together with a host objective'):
        sop.Planner(_exp14(fence=gf, cost=Odd()), backend='nlp')
    qn = sop.Planner(_exp14(), backend='nlp')
    e, g, odd = _exp14(), qn.aircraft, Odd()
    with pytest.raises(NotImplementedError, match='fence together with the host objective'):
        odc.Problem(lambda f: odd.cost(f, qn), lambda f: odd.cost_grad(f, qn), g.get_eom(e.wind), g._state_symbols, qn.num_nodes, qn.time_step,
                    known_parameter_map={}, instance_constraints=qn._instance_constraints, bounds=qn._bounds, fence=gf)
    with pytest.raises(ValueError, match='fence'):
        sop.Planner(_exp14(fence=np.zeros((3, 3))), backend='nlp')
    # the multi-aircraft planner routes a fenced scenario to the collocation backend (the group entry); keep_out stays refused there
    ms = msc.gvf_trial_3ac
    pts = np.array([p[:2] for p in list(ms.p0s) + list(ms.p1s)], float)
    lo, hi = pts.min(0) - 200.0, pts.max(0) + 200.0
    big = ou.GeoFence([(lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1])])
    m = mop.Planner(type('m_f', (ms,), dict(fence=big)), backend='auto')
    assert isinstance(m.prob, odc.Problem) and m.prob.fence is big and m.prob.n_aircraft == len(ms.p0s)
    with pytest.raises(NotImplementedError, match="backend='fit' cannot hold a geofence"):
        mop.Planner(type('m_f', (ms,), dict(fence=big)), backend='fit')
    with pytest.raises(NotImplementedError, match='keep_out'):
        mop.Planner(type('m_f', (ms,), dict(fence=big, keep_out=[ou.KeepOut((0.0, 0.0), 1.0)])), backend='nlp')
    with pytest.raises(NotImplementedError, match="'dubins' initial guess together with a geofence"):
        sop.Planner(_exp14(fence=gf), backend='nlp').prob.dubins_guess()
