"""GPU: the collocation solve inside a convex polygon (include/d2d.h d2d_nlp_solve_fence, csrc/nlp_kernels.hip FENCE instantiation of
nlp_solve_one: nlp_fence_start / nlp_fence_bad, the edges' terms of nlp_merit, nlp_assemble, nlp_recover_stats and nlp_apply) against its
CPU statement tests/nlp_fence_ref.py and against the SLSQP arbiter tests/golden/nlp_fence_slsqp.npz.

Step by step, on the method of tests/test_gpu_nlp_keepout.py: after each budget (inner_max, outer_max) of nlp_steps_ref.BUDGETS the step
count must be the statement's exactly, and W, the discs' and the edges' duals and 2 rho mult must lie within 1e3 x the floor that the
statement shows against itself when every entry of its start moves by an ulp (nlp_steps_ref.measure on the iterate with the duals under
it, nlp_fence_ref.ext).  Node counts 3, 5, 17, 64, 65, 121 (one free node; the chunk edge; the LDS limit of the cyclic reduction); per
node count an edge that the start's bow crosses, D2D_MAX_FENCE rows of which two are absent, and a fence with a hard disc in one launch
in constant wind, and the first case in the steady shear of nlp_wind_ref.fields() in a second one (a launch has one field).
"""
import os

import numpy as np
import pytest

import nlp_fence_ref as F
import nlp_keepout_ref as K
import nlp_steps_ref as S
import nlp_wind_ref as R
from oracle import nlp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nlp_fence_slsqp.npz')
COST_RTOL = 1e-7                 # the issue's: |cost - statement's| <= 1e-7 relative at the end of a solve
NODE_ATOL = 1e-4                 # and the nodes within 1e-4
KEYS = ('cost', 'feas', 'iters', 'status', 'mult', 'keep_mult', 'fence_mult')


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def _out(W, out):
    res = {k: v.cpu().numpy() for k, v in out.items() if k in KEYS and v is not None}
    res['mult'] = res['mult'].transpose(0, 2, 1)
    return W.cpu().numpy().transpose(0, 2, 1), res


def fence_solve(ctx, rows, W0s, edges, discs=None, field=None, t_start=None, **kw):
    """One d2d_nlp_solve_fence launch: rows (B, stride), W0s B x (N, 5), edges (B, n, 4) or None, discs (B, n, 3) or None -> W (B, N, 5),
    out (numpy; mult (B, N, 3), keep_mult (B, n_keep, N), fence_mult (B, n_edge, N))."""
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    out = ctx.nlp_solve_fence(ctx.dev(np.ascontiguousarray(rows)), W, F.H0, None if edges is None else ctx.dev(np.ascontiguousarray(edges)),
                              discs=None if discs is None else ctx.dev(np.ascontiguousarray(discs)), field=field, t_start=t_start, want_mult=True, **kw)
    ctx.sync()
    return _out(W, out)


def _compare(cases, budget, W, out):
    bad, worst, ratio = [], 0.0, 0.0
    for b, case in enumerate(cases):
        m = S.measure(case, budget)
        info, tol = m['info']['raw'], m['tol']
        head = f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        if int(out['iters'][b]) != info['inner']:
            bad.append(f'{head}: iters {out["iters"][b]}, the statement took {info["inner"]}')
        if int(out['status'][b]) != info['status']:
            bad.append(f'{head}: status {out["status"][b]}, the statement\'s {info["status"]}')
        We = F.ext(W[b], dict(zk=out['keep_mult'][b], zf=out['fence_mult'][b]))
        dW = np.abs(We - m['W'][0])
        err = float(dW.max())
        worst, ratio = max(worst, err), max(ratio, err / tol)
        if not err <= tol:
            i, c = np.unravel_index(np.argmax(dW), dW.shape)
            bad.append(f'{head}: W off by {err:.2e} at row {i}, plane {c}' + (' (the duals of discs and edges)' if i >= W[b].shape[0] else ''))
        em = float(np.abs(2 * info['rho'] * out['mult'][b][1:] - info['mult']).max())
        if not em <= tol * 2 * info['rho']:
            bad.append(f'{head}: multipliers off by {em:.2e} > {tol * 2 * info["rho"]:.2e} (rho {info["rho"]:g})')
        cost, feas = case.fn(W[b])
        if not abs(out['cost'][b] - cost) <= 1e-11 * max(1.0, abs(cost)):
            bad.append(f'{head}: cost {out["cost"][b]!r}, the statement at the same W {cost!r}')
        if not abs(out['feas'][b] - feas) <= 1e-12 * max(1.0, 1.0 / F.H0):
            bad.append(f'{head}: feas {out["feas"][b]!r}, the statement at the same W {feas!r}')
    return bad, worst, ratio


@pytest.mark.parametrize('N', F.STEP_N)
def test_kernel_follows_the_statement_step_by_step(ctx, N):
    L = F.steps_launch(N)
    const = [L[t] for t in F.STEP_TAGS if t != 'shear']
    groups = [(const, None, None), ([L['shear']], R.fields()[F.STEP_FIELD], F.STEP_T_START)]
    bad, worst, ratio = [], 0.0, 0.0
    for budget in S.BUDGETS:
        for got, field, t0 in groups:
            cases = [g[0] for g in got]
            W, out = fence_solve(ctx, np.stack([g[1] for g in got]), [c.W0[0][:N] for c in cases], np.stack([g[3] for g in got]),
                                 np.stack([g[2] for g in got]), field, t0, inner_max=budget[0], outer_max=budget[1])
            bd, w, r = _compare(cases, budget, W, out)
            bad += bd; worst = max(worst, w); ratio = max(ratio, r)
    fl = [S.measure(g[0], b)['floor'] for g in L.values() for b in S.BUDGETS]
    print(f'fence-{N}: floors {min(fl):.1e} .. {max(fl):.1e}, largest |(W, z) - statement| {worst:.2e}, largest error / tol {ratio:.2e}')
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('N', F.FULL_N)
def test_full_solves_vs_the_statement(ctx, N):
    """A GeoFence with a margin whose edge cuts the free plan's bow, alone and with a hard disc on another part of the leg: the
    statement's status and step count, its cost within 1e-7 relative and its nodes within 1e-4, every g > 0, the margin held against
    the user's polygon -- by the nodes, and so by the polyline."""
    import d2d.opty_utils as ou
    got = F.full_launch(N)
    W, out = fence_solve(ctx, np.stack([g[1] for g in got]), [g[2] for g in got], np.stack([g[4] for g in got]), np.stack([g[3] for g in got]))
    for b, (prob, _, W0, dk, ed, gf) in enumerate(got):
        Ws, info = F.solve(prob, W0, dk, ed)
        act = ed[F.present(ed)]
        g = F.g_values(W[b][1:-1], act)
        zf = out['fence_mult'][b][:len(act), 1:-1]
        cl = ou.fence_clearance(gf, W[b][:, 0], W[b][:, 1])
        dact = dk[dk[:, 2] > 0]
        gd = K.g_values(W[b][1:-1], dact)[0] if len(dact) else np.ones((1, 1))
        print(f'{N}-{b}: status {out["status"][b]} / {info["status"]}, cost {out["cost"][b]:.12f} vs {info["cost"]:.12f}, steps {out["iters"][b]} / {info["inner"]}, '
              f'|W - statement| {np.abs(W[b] - Ws).max():.1e}, feas {out["feas"][b]:.1e}, min g {g.min():.1e}, largest edge dual {zf.max():.3g} / {info["zf"].max():.3g}, '
              f'largest disc dual {out["keep_mult"][b].max():.3g} / {info["zk"].max():.3g}, clearance {min(cl):.6f} (margin {gf.margin:.6f})')
        assert out['status'][b] == info['status'] == 1 and out['iters'][b] == info['inner']
        assert abs(out['cost'][b] - info['cost']) <= COST_RTOL * abs(info['cost'])
        assert np.abs(W[b] - Ws).max() <= NODE_ATOL
        assert out['feas'][b] <= 1e-9 and g.min() > 0.0 and gd.min() > 0.0
        assert min(cl) >= gf.margin
        assert zf.max() > 1e-2 and (not len(dact) or out['keep_mult'][b].max() > 1e-2)       # both bind (nlp_fence_ref.FULL_PAR)
        assert np.abs(zf * g - nlp.MUB_MIN).max() <= 1e-7
        assert not out['fence_mult'][b][:, [0, -1]].any() and not out['fence_mult'][b][len(act):].any()
        assert abs(out['cost'][b] - prob.cost(W[b])) <= 1e-11 * max(1.0, out['cost'][b])          # the edges add nothing to the cost


def test_device_refusals(ctx):
    """One launch with every cause of a refusal, a good problem in front, between and behind: status 3, NaN cost and feas, no step, W
    untouched; the good problems solved alike.  n_edge = 9 and a missing table are D2D_EINVAL."""
    import d2dhip
    prob, r, W0, dk, ed, gf = F.full_launch(41)[0]
    pb = prob.pb
    p0, ax, nrm, ll = F.leg_frame(pb)

    def edge(a, p, kap=0.1):
        a = np.asarray(a, float)
        return (a[0], a[1], float(a @ p), kap)
    nan = ed.copy(); nan[5] = (0.0, 0.0, np.nan, 0.0)                      # a non-finite entry, even of an absent row
    inf = ed.copy(); inf[1, 2] = np.inf
    long_ = ed.copy(); long_[2, :2] *= 1.0 + 1e-9                          # |a| off 1
    kap0 = ed.copy(); kap0[0, 3] = 0.0
    kapn = ed.copy(); kapn[3, 3] = -1.0
    end0 = ed.copy(); end0[4] = edge(-ax, p0 + 0.01 * ll * ax)             # p0 outside
    end1 = ed.copy(); end1[4] = edge(ax, p0 + ll * ax)                     # p1 ON the edge: g = 0
    # two edges that face each other 1e-3 apart round the axis with kap = 1: each pass pushes a node out of the other one
    shut = ed.copy(); shut[4] = (nrm[0], nrm[1], float(nrm @ p0) + 5e-4, 1.0); shut[5] = (-nrm[0], -nrm[1], -float(nrm @ p0) + 5e-4, 1.0)
    # a disc the fence's start rule pushes a node into: the disc lies just inside the left edge, where the bowed start is pushed to
    bad = [nan, inf, long_, kap0, kapn, end0, end1, shut]
    tabs = [ed]
    for t in bad:
        tabs += [t, ed]
    B = len(tabs)
    W0b = W0.copy(); W0b[:, :2] += (0.2 * ll * np.sin(np.pi * np.linspace(0, 1, pb.N)))[:, None] * nrm     # the start outside the fence: moved in
    W0s = [W0b] * B
    W, out = fence_solve(ctx, np.stack([r] * B), W0s, np.stack(tabs), np.stack([dk] * B))
    print(f'status {out["status"].tolist()}')
    for b in range(B):
        info = F.solve(prob, W0s[b], dk, tabs[b])[1]
        if b % 2:
            assert out['status'][b] == d2dhip.ST_NONFINITE == info['status'] and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and out['iters'][b] == 0, b
            assert np.array_equal(W[b], W0s[b]), b
        else:
            assert out['status'][b] == 1 == info['status'] and np.array_equal(W[b], W[0]) and out['cost'][b] == out['cost'][0], b
    assert abs(out['cost'][0] - F.solve(prob, W0b, dk, ed)[1]['cost']) <= COST_RTOL * out['cost'][0]
    with pytest.raises(d2dhip.D2DError, match=rf'error -1: .*n_edge = {d2dhip.MAX_FENCE + 1} outside'):       # D2D_EINVAL
        fence_solve(ctx, r[None], [W0], np.zeros((1, d2dhip.MAX_FENCE + 1, 4)))
    lib = ctx.lib
    import ctypes as C
    Wd = ctx.dev(np.ascontiguousarray(W0.T[None])); work = ctx.empty(lib.d2d_nlp_workspace_doubles(pb.N)); cost = ctx.empty(1); feas = ctx.empty(1)
    keep = d2dhip.KeepOutC(0, 0, None)
    args = [ctx.h, 1, pb.N, F.H0, ctx.dev(r[None]).data_ptr(), None, Wd.data_ptr(), work.data_ptr(), None, cost.data_ptr(), feas.data_ptr(), None, None, None,
            None, C.byref(keep), None]
    assert lib.d2d_nlp_solve_fence(*args, None, None) == -1                                       # fence NULL
    assert lib.d2d_nlp_solve_fence(*args, C.byref(d2dhip.FenceC(4, 0, None)), work.data_ptr()) == -1   # edges NULL with n_edge > 0
    assert lib.d2d_nlp_solve_fence(*args, C.byref(d2dhip.FenceC(4, 0, work.data_ptr())), None) == -1   # fwork NULL with n_edge > 0
    assert lib.d2d_nlp_solve_fence(*args, C.byref(d2dhip.FenceC(-1, 0, None)), None) == -1
    ctx.sync()
    assert np.array_equal(Wd.cpu().numpy()[0].T, W0)


def test_disc_in_the_way_of_the_start_rule_refuses(ctx):
    """A free node with g <= 0 at a DISC after the edges' start rule: the bowed start is pushed in to g = kap of the left edge, where a hard
    disc sits that the discs' rule, which comes first, has not seen the node in."""
    import d2dhip
    prob, r, W0, dk, ed, gf = F.full_launch(41)[0]
    pb = prob.pb
    p0, ax, nrm, ll = F.leg_frame(pb)
    k = int(np.argmax(ed[:4, :2] @ nrm))                                   # the left edge
    left = float(ed[k, 2] - ed[k, :2] @ p0)                                # its distance from the axis
    W0b = W0.copy(); W0b[:, :2] += (0.2 * ll * np.sin(np.pi * np.linspace(0, 1, pb.N)))[:, None] * nrm
    c = p0 + 0.5 * ll * ax + (left - ed[k, 3]) * nrm                       # where the start rule puts the middle node
    discs = K.pad([(c[0], c[1], 0.3 * ed[k, 3])])
    W, out = fence_solve(ctx, np.stack([r, r]), [W0b, W0b], np.stack([ed, ed]), np.stack([discs, dk]))
    info = F.solve(prob, W0b, discs, ed)[1]
    assert out['status'].tolist() == [d2dhip.ST_NONFINITE, 1] and info['status'] == d2dhip.ST_NONFINITE
    assert np.array_equal(W[0], W0b) and np.isnan(out['cost'][0])


def test_order_only_schedules(ctx):
    import torch
    got = F.full_launch(41)
    rows, W0s = np.stack([g[1] for g in got] * 3), [g[2] for g in got] * 3
    discs, edges = np.stack([g[3] for g in got] * 3), np.stack([g[4] for g in got] * 3)
    W, out = fence_solve(ctx, rows, W0s, edges, discs)
    order = torch.tensor([5, 3, 1, 0, 2, 4], dtype=torch.int32, device=ctx.device)
    Wo, oo = fence_solve(ctx, rows, W0s, edges, discs, order=order, slots=2)
    assert np.array_equal(W, Wo)
    for k in KEYS:
        assert np.array_equal(out[k], oo[k]), k


def _keep_solve(ctx, rows, W0s, discs, field=None, t_start=None):
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    out = ctx.nlp_solve_keepout(ctx.dev(np.ascontiguousarray(rows)), W, F.H0, None if discs is None else ctx.dev(np.ascontiguousarray(discs)),
                                field=field, t_start=t_start, want_mult=True)
    ctx.sync()
    return _out(W, out)


@pytest.mark.parametrize('N, shear', [(17, False), (41, False), (17, True)])
def test_no_edges_is_the_keepout_solve_and_the_plain_solve_bit_for_bit(ctx, N, shear):
    """n_edge = 0 (edges None): the bytes of d2d_nlp_solve_keepout on the same discs -- W, cost, feas, iters, status, the equalities'
    multipliers and the discs' -- and with n_keep = 0 too those of d2d_nlp_solve (d2d_nlp_solve_wind in the shear).  D2D_MAX_FENCE rows
    that are all absent give the same bytes through the fence kernel itself."""
    field, t0 = (R.fields()['shear'], 1.5) if shear else (None, None)
    got = K.full_launch(N)
    rows, W0s, discs = np.stack([g[1] for g in got]), [g[2] for g in got], np.stack([g[3] for g in got])
    Wk, ok = _keep_solve(ctx, rows, W0s, discs, field, t0)
    for edges in (None, np.zeros((len(got), F.MAX_FENCE, 4))):
        Wf, of = fence_solve(ctx, rows, W0s, edges, discs, field, t0)
        assert np.array_equal(Wf, Wk)
        for k in ('cost', 'feas', 'iters', 'status', 'mult', 'keep_mult'):
            assert np.array_equal(of[k], ok[k], equal_nan=True), (k, edges is None)
        assert 'fence_mult' not in of or not of['fence_mult'].any()
    Wd = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    op = (ctx.nlp_solve_wind(ctx.dev(rows), Wd, F.H0, field, t0, want_mult=True) if shear else ctx.nlp_solve(ctx.dev(rows), Wd, F.H0, want_mult=True))
    ctx.sync()
    Wp, op = _out(Wd, op)
    for edges in (None, np.zeros((len(got), F.MAX_FENCE, 4))):
        Wf, of = fence_solve(ctx, rows, W0s, edges, None, field, t0)
        assert np.array_equal(Wf, Wp)
        for k in ('cost', 'feas', 'iters', 'status', 'mult'):
            assert np.array_equal(of[k], op[k], equal_nan=True), (k, edges is None)
        assert 'keep_mult' not in of


def test_against_the_slsqp_arbiter(ctx):
    """The kernel against scipy SLSQP with the node inequalities as true constraints (tests/golden/make_nlp_fence_golden.py): the cost
    to tests/test_nlp_fence_cpu.py's tolerance, ten times the statement's largest difference over these cases; in the case with two
    binding edges and in the one with an edge and a disc both carry duals > 1e-3."""
    from test_nlp_fence_cpu import SLSQP_COST_RTOL
    g = np.load(GOLDEN)
    for k, name in enumerate(F.ARB_CASES):
        N, discs, edges = int(g[f'c{k}_N']), g[f'c{k}_discs'], g[f'c{k}_edges']
        W, out = fence_solve(ctx, g[f'c{k}_row'][None], [g[f'c{k}_W0']], edges[None], discs[None] if len(discs) else None)
        dc = abs(out['cost'][0] - g[f'c{k}_cost']) / g[f'c{k}_cost']
        gf = F.g_values(W[0][1:-1], edges)
        zmax = out['fence_mult'][0].max(1)
        print(f'case {k} {name} (N {N}): status {out["status"][0]}, cost off by {dc:.2e} relative, feas {out["feas"][0]:.1e}, min g {gf.min():.1e}, '
              f'edge duals {np.array2string(zmax, precision=3)}')
        assert out['status'][0] == 1 and out['feas'][0] <= 1e-9 and gf.min() > 0.0
        assert dc <= SLSQP_COST_RTOL
        if name.startswith('roof'):
            assert (zmax > 1e-3).sum() == 2
        if name.startswith('mixed'):
            assert (zmax > 1e-3).sum() == 1 and out['keep_mult'][0].max() > 1e-3
            assert K.g_values(W[0][1:-1], discs)[0].min() > 0.0


def test_plan_batch_returns_the_direct_solve(ctx):
    """full_sim.plan_batch(backend='nlp', fence=): one GeoFence for all problems, one per problem and the lowered rows, with and without
    keep_out's discs, give the bytes of Context.nlp_solve_fence on the same rows."""
    import full_sim
    got = F.full_launch(41)
    rows, W0s = np.stack([g[1] for g in got]), np.stack([g[2].T for g in got])
    gf = got[0][5]
    T = (41 - 1) * F.H0
    for discs in (None, np.stack([got[1][3][:1]] * 2)):
        W, out = fence_solve(ctx, rows, [g[2] for g in got], np.stack([gf.lowered()] * 2), discs)
        for fence in (gf, [gf, gf], np.stack([gf.lowered()] * 2)):
            pl = full_sim.plan_batch(rows, 41, T, 1.0, backend='nlp', W0=W0s, h=F.H0, fence=fence, keep_out=discs, want_mult=True)
            ctx.sync()
            assert pl['entry'] == 'nlp_solve_fence' and np.array_equal(pl['W'].cpu().numpy().transpose(0, 2, 1), W)
            assert np.array_equal(pl['fence_mult'].cpu().numpy(), out['fence_mult']) and np.array_equal(pl['cost'].cpu().numpy(), out['cost'])
            assert np.array_equal(pl['fence'], np.stack([gf.lowered()] * 2)) and (pl['status'].cpu().numpy() == 1).all()
            assert (discs is None) == ('keep' not in pl)


def test_planners_plan_a_scenario_with_a_fence(ctx):
    """single_opt_planner.Planner on exp_14 inside a corridor that leaves 0.8 of the free plan's largest excursion from the leg's axis, with
    a margin of 0.5 m: backend 'auto' goes to 'nlp', the plan converges, info['fence_clearance'] >= margin where the free plan's is not,
    and the plan is Context.nlp_solve_fence's on the same row, start and lowered rows; opty's Problem(fence=) built by hand gives the
    same.  multi_opt_planner.Planner on a two-aircraft scenario inside a polygon goes through the group entry."""
    import d2d.optyplan_scenarios as sc
    import d2d.multioptyplan_scenarios as msc
    import d2d.opty_utils as ou
    import multi_opt_planner as mop
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    from test_nlp_fence_cpu import _exp14, scenario_fence
    q = sop.Planner(_exp14(), backend='nlp'); q.run(q.get_initial_guess())
    e = sc.exp_14
    p0, p1 = np.array(e.p0[:2], float), np.array(e.p1[:2], float)
    ax = (p1 - p0) / np.hypot(*(p1 - p0)); nrm = np.array([-ax[1], ax[0]])
    lat = (np.stack([q.sol_x, q.sol_y], 1) - p0) @ nrm
    up = lat.max() >= -lat.min()
    cut, m = 0.8 * float(np.abs(lat).max()), 0.5
    gf = scenario_fence(e, cut + m if up else 200.0, 200.0 if up else cut + m, m)
    assert min(ou.fence_clearance(gf, q.sol_x, q.sol_y)) < m
    p = sop.Planner(_exp14(fence=gf), backend='auto')
    x0 = p.get_initial_guess()
    p.run(x0)
    cl = p.info['fence_clearance']
    print(f'exp_14 inside {gf}: status {p.info["status"]}, clearance {min(cl):.6f} (margin {m}), free plan {min(ou.fence_clearance(gf, q.sol_x, q.sol_y)):.3f}, '
          f'cost {p.info["obj_val"]:.9f} (free {q.info["obj_val"]:.9f}), steps {p.info["iters"]}')
    assert p.info['backend_used'] == 'nlp' and p.info['status'] == 1, p.info
    assert len(cl) == 4 and min(cl) >= m and min(cl) <= m + 1e-6                     # held, and binding
    assert 'fence_clearance' not in q.info
    N = p.num_nodes
    rows, _ = p.prob._rows()
    W0 = np.stack([x0[s] for s in (p._slice_x, p._slice_y, p._slice_psi, p._slice_phi, p._slice_v)], 1)
    W = ctx.dev(np.ascontiguousarray(W0.T[None]))
    out = ctx.nlp_solve_fence(ctx.dev(rows), W, p.time_step, ctx.dev(gf.lowered()[None]), **p.prob._solver_kw())
    ctx.sync()
    Wh = W.cpu().numpy()[0]
    assert int(out['status'][0].item()) == 1 and np.array_equal(Wh[0], p.sol_x) and np.array_equal(Wh[1], p.sol_y) and np.array_equal(Wh[4], p.sol_v)
    g, cost = p.aircraft, e.cost
    pr = odc.Problem(lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q), g.get_eom(e.wind), g._state_symbols, N, p.time_step,
                     known_parameter_map={}, instance_constraints=p._instance_constraints, bounds=p._bounds, fence=gf)
    sol, info = pr.solve(x0)
    assert np.array_equal(sol, p.solution) and info['fence_clearance'] == cl
    # several aircraft: the group entry, every aircraft inside
    ms = msc.gvf_trial_3ac
    pts = np.array([pp[:2] for pp in list(ms.p0s) + list(ms.p1s)], float)
    lo, hi = pts.min(0) - 200.0, pts.max(0) + 200.0
    big = ou.GeoFence([(lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1])], 1.0)
    mf = mop.Planner(type('m_f', (ms,), dict(fence=big)), backend='nlp'); mf.run()
    m0 = mop.Planner(ms, backend='nlp'); m0.run()
    fc = mf.info['fence_clearance']
    print(f'{ms.__name__} inside {big}: status {mf.info["status"]}, sweeps {mf.info["sweeps"]}, smallest clearance {min(min(c) for c in fc):.3f}')
    assert len(fc) == len(ms.p0s) and min(min(c) for c in fc) >= 1.0 and mf.info['backend_used'] == 'nlp'
    print(f'status {mf.info["status"]} / {m0.info["status"]}, cost {mf.info["obj_val"]!r} / {m0.info["obj_val"]!r}')
    # (200 m from every end pose the edges' barrier, mub / g <= 1e-9 / 100, moves nothing that the tolerances see)
    assert mf.info['status'] == m0.info['status'] == [1] * len(ms.p0s)
    assert abs(mf.info['obj_val'] - m0.info['obj_val']) <= 1e-6 * abs(m0.info['obj_val'])
