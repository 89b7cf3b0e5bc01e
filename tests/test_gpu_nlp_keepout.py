"""GPU: the collocation solve outside hard keep-out discs (include/d2d.h d2d_nlp_solve_keepout, csrc/nlp_kernels.hip KEEP instantiation of
nlp_solve_one: nlp_keep_start / nlp_keep_bad, the discs' terms of nlp_merit, nlp_assemble, nlp_recover_stats and nlp_apply) against its
CPU statement tests/nlp_keepout_ref.py and against the SLSQP arbiter tests/golden/nlp_keepout_slsqp.npz.

Step by step, on the method of tests/test_gpu_nlp_free.py: after each budget (inner_max, outer_max) of nlp_steps_ref.BUDGETS the step
count must be the statement's exactly, and W, the discs' duals and 2 rho mult must lie within 1e3 x the floor that the statement shows
against itself when every entry of its start moves by an ulp (nlp_steps_ref.measure on the iterate with the duals under it,
nlp_keepout_ref.ext).  Node counts 3, 5, 17, 64, 65, 121, 122, 129 (one free node; the chunk edge; the LDS limit of the cyclic
reduction; a ragged last chunk); per node count a binding disc in constant wind, two overlapping discs with a y box and D2D_MAX_KEEP
rows of which two are absent and six far away in one launch, and the binding disc in the steady shear of nlp_wind_ref.fields() in a
second one (a launch has one field).

Measured on the run that added this module (MI355X), per node count over its four cases and the eight budgets: the statement's floors,
the largest |(W, z)_kernel - statement| and the largest error / tolerance (the share of the 1e3 margin the kernel uses):
  3 nodes        floors 1.4e-17 .. 9.1e-12   error 1.4e-11   error / tol 1.0e-02
  5 nodes        floors 1.1e-16 .. 7.7e-12   error 6.4e-12   error / tol 1.0e-02
  17 nodes       floors 1.8e-15 .. 6.7e-12   error 3.1e-12   error / tol 1.0e-02
  64 nodes       floors 7.1e-15 .. 5.6e-12   error 1.1e-11   error / tol 1.2e-02
  65 nodes       floors 7.1e-15 .. 8.9e-12   error 9.9e-12   error / tol 1.7e-02
  121 nodes      floors 5.2e-14 .. 5.0e-12   error 4.0e-12   error / tol 4.9e-03
  122 nodes      floors 7.8e-14 .. 9.4e-12   error 3.8e-12   error / tol 1.9e-03
  129 nodes      floors 5.7e-14 .. 8.9e-12   error 5.6e-12   error / tol 2.2e-03
Every step count and multiplier agreed.
Power of the comparison, same run, the 17-node launches against two local builds that were not committed:
  - z I dropped from the Newton block: the FIRST budget already fails,
      'keep-17-bind (1, 1): floor 6.1e-14, tol 6.1e-11: W off by 6.95e-03 at row 18, plane 3 (the discs' duals)'
      'keep-17-two (1, 1): floor 1.3e-13, tol 1.3e-10: W off by 4.38e-03 at row 18, plane 3 (the discs' duals)'
    and every later budget with it (largest |(W, z) - statement| 2.06, largest error / tol 5.3e+10);
  the linearised ratio test tau g / (-2 d.s) in the place of the quadratic's root: the budgets of one outer iteration still PASS (in
    these cases another limit binds first in the early steps: the linear test only bites where it is the shortest), budget (5, 4) fails,
      'keep-17-shear (5, 4): floor 3.9e-14, tol 3.9e-11: W off by 2.35e-03 at row 18, plane 2 (the discs' duals)'
    (largest error / tol 6.0e+07).
"""
import os

import numpy as np
import pytest

import nlp_keepout_ref as K
import nlp_steps_ref as S
import nlp_wind_ref as R
from oracle import nlp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nlp_keepout_slsqp.npz')
COST_RTOL = 1e-7                 # tests/test_gpu_nlp.py: |cost - statement's| <= 1e-7 max(cost, 1e-3) at the end of a solve


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def keep_solve(ctx, rows, W0s, discs, field=None, t_start=None, bounds=None, **kw):
    """One d2d_nlp_solve_keepout launch: rows (B, stride), W0s B x (N, 5), discs (B, n, 3) or None -> W (B, N, 5), out (numpy; mult
    (B, N, 3), keep_mult (B, n, N))."""
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    out = ctx.nlp_solve_keepout(ctx.dev(np.ascontiguousarray(rows)), W, K.H0, None if discs is None else ctx.dev(np.ascontiguousarray(discs)),
                                field=field, t_start=t_start, want_mult=True, bounds=None if bounds is None else ctx.dev(np.ascontiguousarray(bounds)), **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in ('cost', 'feas', 'iters', 'status', 'mult', 'keep_mult') and v is not None}
    res['mult'] = res['mult'].transpose(0, 2, 1)
    return W.cpu().numpy().transpose(0, 2, 1), res


def _compare(cases, budget, W, out):
    bad, worst, ratio = [], 0.0, 0.0
    for b, case in enumerate(cases):
        m = S.measure(case, budget)
        info, tol = m['info']['raw'], m['tol']
        head = f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        if int(out['iters'][b]) != info['inner']:
            bad.append(f'{head}: iters {out["iters"][b]}, the statement took {info["inner"]}')
        We = K.ext(W[b], dict(zk=out['keep_mult'][b]))
        dW = np.abs(We - m['W'][0])
        err = float(dW.max())
        worst, ratio = max(worst, err), max(ratio, err / tol)
        if not err <= tol:
            i, c = np.unravel_index(np.argmax(dW), dW.shape)
            bad.append(f'{head}: W off by {err:.2e} at row {i}, plane {c}' + (' (the discs\' duals)' if i >= W[b].shape[0] else ''))
        em = float(np.abs(2 * info['rho'] * out['mult'][b][1:] - info['mult']).max())
        if not em <= tol * 2 * info['rho']:
            bad.append(f'{head}: multipliers off by {em:.2e} > {tol * 2 * info["rho"]:.2e} (rho {info["rho"]:g})')
        cost, feas = case.fn(W[b])
        if not abs(out['cost'][b] - cost) <= 1e-11 * max(1.0, abs(cost)):
            bad.append(f'{head}: cost {out["cost"][b]!r}, the statement at the same W {cost!r}')
        if not abs(out['feas'][b] - feas) <= 1e-12 * max(1.0, 1.0 / K.H0):
            bad.append(f'{head}: feas {out["feas"][b]!r}, the statement at the same W {feas!r}')
    return bad, worst, ratio


@pytest.mark.parametrize('N', K.STEP_N)
def test_kernel_follows_the_statement_step_by_step(ctx, N):
    L = K.steps_launch(N)
    const = [L[t] for t in K.STEP_TAGS if t != 'shear']
    groups = [(const, None, None), ([L['shear']], R.fields()[K.STEP_FIELD], K.STEP_T_START)]
    bad, worst, ratio = [], 0.0, 0.0
    for budget in S.BUDGETS:
        for got, field, t0 in groups:
            cases = [g[0] for g in got]
            W, out = keep_solve(ctx, np.stack([g[1] for g in got]), [c.W0[0][:N] for c in cases], np.stack([g[2] for g in got]), field, t0,
                                inner_max=budget[0], outer_max=budget[1])
            bd, w, r = _compare(cases, budget, W, out)
            bad += bd; worst = max(worst, w); ratio = max(ratio, r)
    fl = [S.measure(g[0], b)['floor'] for g in L.values() for b in S.BUDGETS]
    print(f'keep-{N}: floors {min(fl):.1e} .. {max(fl):.1e}, largest |(W, z) - statement| {worst:.2e}, largest error / tol {ratio:.2e}')
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('N', K.FULL_N)
def test_full_solves_vs_the_statement(ctx, N):
    """One disc, and the same with a second one that closes the near side: the statement's verdict and cost, feas <= 1e-9, every free
    node outside, the disc binding with a dual that counts, complementarity at the barrier's floor, the margin asked held by the
    polyline -- and the soft-cost solve of the same rows (d2d_nlp_solve) through the disc: the case this entry exists for."""
    got = K.full_launch(N)
    rows, W0s, discs = np.stack([g[1] for g in got]), [g[2] for g in got], np.stack([g[3] for g in got])
    W, out = keep_solve(ctx, rows, W0s, discs)
    Wd = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    soft = ctx.nlp_solve(ctx.dev(rows), Wd, K.H0)
    ctx.sync()
    Ws = Wd.cpu().numpy().transpose(0, 2, 1)
    for b, (prob, _, W0, dk, (c, ru, margin)) in enumerate(got):
        _, info = K.solve(prob, W0, dk)
        act = dk[dk[:, 2] > 0]
        gk = K.g_values(W[b][1:-1], act)[0]
        zk = out['keep_mult'][b][:len(act), 1:-1]
        k = np.unravel_index(np.argmin(gk / act[:, 2:3] ** 2), gk.shape)
        cl, cls = K.polyline_clearance(W[b][:, :2], c, ru), K.polyline_clearance(Ws[b][:, :2], c, ru)
        print(f'{N}-{b}: status {out["status"][b]} / {info["status"]}, cost {out["cost"][b]:.12f} vs {info["cost"]:.12f}, steps {out["iters"][b]} / {info["inner"]}, '
              f'feas {out["feas"][b]:.1e}, min g / R^2 {gk[k] / act[k[0], 2] ** 2:.1e} with z / zmax {zk[k] / zk.max():.2f}, |z g - mub| {np.abs(zk * gk - nlp.MUB_MIN).max():.1e}, '
              f'clearance {cl:.4f} (margin {margin:.4f}); soft cost: status {int(soft["status"][b].item())}, clearance {cls:.4f}')
        assert out['status'][b] == info['status'] == 1
        assert abs(out['cost'][b] - info['cost']) <= COST_RTOL * max(info['cost'], 1e-3)
        assert out['feas'][b] <= 1e-9 and gk.min() >= 0.0
        assert gk[k] / act[k[0], 2] ** 2 < 1e-6 and zk[k] > 1e-3 * zk.max()
        assert np.abs(zk * gk - nlp.MUB_MIN).max() <= 1e-7
        assert not out['keep_mult'][b][:, [0, -1]].any() and not out['keep_mult'][b][len(act):].any()
        assert cl >= margin
        assert int(soft['status'][b].item()) == 1 and cls < 0.0
        assert abs(out['cost'][b] - prob.cost(W[b])) <= 1e-11 * max(1.0, out['cost'][b])          # the discs add nothing to the cost


def _plain_rows(N=41):
    got = [S.plain_case(N, tag, 0) for tag in ('disc1', 'windbox')]
    return np.stack([g[1] for g in got]), [g[0].W0[0] for g in got]


def test_no_discs_is_the_plain_solve_bit_for_bit(ctx):
    """n_keep = 0 (discs None), with and without a field: W, cost, iters and status of d2d_nlp_solve / d2d_nlp_solve_wind on the same rows."""
    rows, W0s = _plain_rows()
    Wk, ok = keep_solve(ctx, rows, W0s, None)
    Wd = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    op = ctx.nlp_solve(ctx.dev(rows), Wd, K.H0)
    ctx.sync()
    assert np.array_equal(Wk, Wd.cpu().numpy().transpose(0, 2, 1)) and (ok['status'] == 1).all()
    for k in ('cost', 'iters', 'status'):
        assert np.array_equal(ok[k], op[k].cpu().numpy()), k
    F = R.fields()['shear']
    Wk, ok = keep_solve(ctx, rows, W0s, None, F, 1.5)
    Wd = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    op = ctx.nlp_solve_wind(ctx.dev(rows), Wd, K.H0, F, 1.5)
    ctx.sync()
    assert np.array_equal(Wk, Wd.cpu().numpy().transpose(0, 2, 1))
    for k in ('cost', 'iters', 'status'):
        assert np.array_equal(ok[k], op[k].cpu().numpy()), k
    assert 'keep_mult' not in ok                # (keep_solve drops the entries that are None: without discs there are no duals)


def test_order_only_schedules_and_bounds_are_honoured(ctx):
    import torch
    got = K.full_launch(41)
    rows, W0s, discs = np.stack([g[1] for g in got] * 3), [g[2] for g in got] * 3, np.stack([g[3] for g in got] * 3)
    W, out = keep_solve(ctx, rows, W0s, discs)
    order = torch.tensor([5, 3, 1, 0, 2, 4], dtype=torch.int32, device=ctx.device)
    Wo, oo = keep_solve(ctx, rows, W0s, discs, order=order, slots=2)
    assert np.array_equal(W, Wo)
    for k in ('cost', 'feas', 'iters', 'status', 'keep_mult', 'mult'):
        assert np.array_equal(out[k], oo[k]), k
    # d2d_nlp_opts.bounds: phi in [-25, +35] deg on the first problem only (the free plan banks to both limits of 35 deg; the statement
    # converges with -25 and stalls below -20): the statement with the same interval agrees, the plan holds it
    bnd = np.zeros((6, 4)); bnd[0, :2] = (-np.deg2rad(25.0), np.deg2rad(35.0))
    Wb, ob = keep_solve(ctx, rows, W0s, discs, bounds=bnd)
    prob, _, W0, dk, _ = got[0]
    import copy
    pb = copy.deepcopy(prob.pb); pb.lo[:, 3], pb.hi[:, 3] = bnd[0, 0], bnd[0, 1]
    _, info = K.solve(K.Plain(pb), W0, dk)
    print(f'bounds: status {ob["status"][0]} / {info["status"]}, cost {ob["cost"][0]:.12f} vs {info["cost"]:.12f} (free: {out["cost"][0]:.12f}), min phi {Wb[0][:, 3].min():.6f}')
    assert ob['status'][0] == info['status'] == 1 and abs(ob['cost'][0] - info['cost']) <= COST_RTOL * max(info['cost'], 1e-3)
    assert Wb[0][:, 3].min() > bnd[0, 0] and W[0][:, 3].min() < bnd[0, 0]            # the interval binds: the free plan leaves it
    assert np.array_equal(Wb[1], W[1])


def test_against_the_slsqp_arbiter(ctx):
    """The kernel against scipy SLSQP with the node inequalities as true constraints (5, 9, 17 nodes, one and two discs): the cost to
    tests/test_nlp_keepout_cpu.py's tolerance, measured there on the statement: 10 x its largest difference over these cases."""
    from test_nlp_keepout_cpu import SLSQP_COST_RTOL
    g = np.load(GOLDEN)
    for k in range(int(g['n_cases'])):
        N, discs = int(g[f'c{k}_N']), g[f'c{k}_discs']
        W, out = keep_solve(ctx, g[f'c{k}_row'][None], [g[f'c{k}_W0']], discs[None])
        dc = abs(out['cost'][0] - g[f'c{k}_cost']) / g[f'c{k}_cost']
        gk = K.g_values(W[0][1:-1], discs)[0]
        print(f'case {k} (N {N}, {len(discs)} discs): status {out["status"][0]}, cost off by {dc:.2e} relative, feas {out["feas"][0]:.1e}, min g {gk.min():.1e}')
        assert out['status'][0] == 1 and out['feas'][0] <= 1e-9 and gk.min() >= 0.0
        assert dc <= SLSQP_COST_RTOL


def test_device_refusals(ctx):
    """An end pose inside a disc, a NaN radius and discs that cover the y box: status 3, NaN cost and feas, W untouched, each between two
    neighbours that are solved; n_keep = 9 is D2D_EINVAL."""
    import d2dhip
    prob, r, W0, dk, _ = K.full_launch(41)[0]
    pbb, rb, W0b, Lb = K.leg_problem(41, 0, y_box=True)
    inside = dk.copy(); inside[1] = (prob.pb.p1[0] + 0.5, prob.pb.p1[1], 1.0)
    nanr = dk.copy(); nanr[3] = (1e3, 1e3, np.nan)
    cover = K.pad([(0.5 * Lb, 0.0, 0.3 * Lb)])
    rows = np.stack([r, r, r, r, rb, r])
    W0s = [W0, W0, W0, W0, W0b, W0]
    discs = np.stack([dk, inside, dk, nanr, cover, dk])
    W, out = keep_solve(ctx, rows, W0s, discs)
    print(f'status {out["status"].tolist()}, cost {out["cost"].tolist()}')
    for b in (1, 3, 4):
        assert out['status'][b] == d2dhip.ST_NONFINITE and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and out['iters'][b] == 0
        assert np.array_equal(W[b], W0s[b])
        assert K.solve(K.Plain(pbb) if b == 4 else prob, W0s[b], discs[b])[1]['status'] == K.ST_NONFINITE
    for b in (0, 2, 5):
        assert out['status'][b] == 1 and np.array_equal(W[b], W[0]) and out['cost'][b] == out['cost'][0]
    with pytest.raises(d2dhip.D2DError, match=rf'error -1: .*n_keep = {d2dhip.MAX_KEEP + 1} outside'):       # D2D_EINVAL
        keep_solve(ctx, rows[:1], W0s[:1], np.zeros((1, d2dhip.MAX_KEEP + 1, 3)))


def test_host_routes_return_the_direct_solve(ctx):
    """single_opt_planner.Planner on exp_14 with one KeepOut across the leg, opty.direct_collocation.Problem(keep_out=) and
    full_sim.plan_batch(keep_out=) return the plan of Context.nlp_solve_keepout on the same row, start and lowered disc."""
    import d2d.optyplan_scenarios as sc
    import d2d.opty_utils as ou
    import full_sim
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    from test_nlp_keepout_cpu import _disc_across, _exp14
    ko = _disc_across(sc.exp_14)
    p = sop.Planner(_exp14(keep_out=[ko]), backend='auto')
    x0 = p.get_initial_guess()
    p.run(x0)
    assert p.info['backend_used'] == 'nlp' and p.info['status'] == 1, p.info
    cl = p.info['keep_out_clearance']
    print(f'exp_14 round {ko}: clearance {cl}, cost {p.info["obj_val"]:.9f}, steps {p.info["iters"]}')
    assert len(cl) == 1 and cl[0] >= ko.margin
    assert abs(cl[0] - K.polyline_clearance(np.stack([p.sol_x, p.sol_y], 1), ko.c, ko.r)) <= 1e-12
    # without the list the scenario plans as before, and its info has no such key
    q = sop.Planner(_exp14(), backend='nlp'); q.run(q.get_initial_guess())
    assert 'keep_out_clearance' not in q.info and ou.keep_out_clearance([ko], q.sol_x, q.sol_y)[0] < ko.margin
    # the direct solve
    N = p.num_nodes
    rows, _ = p.prob._rows()
    W0 = np.stack([x0[s] for s in (p._slice_x, p._slice_y, p._slice_psi, p._slice_phi, p._slice_v)], 1)
    kw = p.prob._solver_kw()
    W = ctx.dev(np.ascontiguousarray(W0.T[None]))
    dsc = ctx.dev(rows)
    out = ctx.nlp_solve_keepout(dsc, W, p.time_step, ctx.dev(p.prob.keep_rows[None]), **kw)
    ctx.sync()
    Wh = W.cpu().numpy()[0]
    assert int(out['status'][0].item()) == 1
    assert np.array_equal(Wh[0], p.sol_x) and np.array_equal(Wh[1], p.sol_y) and np.array_equal(Wh[4], p.sol_v)
    # Problem(keep_out=) built by hand
    e, g = _exp14(), p.aircraft
    cost = e.cost
    pr = odc.Problem(lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q), g.get_eom(e.wind), g._state_symbols, N, p.time_step,
                     known_parameter_map={}, instance_constraints=p._instance_constraints, bounds=p._bounds, keep_out=[ko])
    sol, info = pr.solve(x0)
    assert np.array_equal(sol, p.solution) and info['keep_out_clearance'] == cl
    # plan_batch: the lowered table, and the list
    for keep in (p.prob.keep_rows[None], [ko]):
        pl = full_sim.plan_batch(rows, N, p.duration, e.obj_scale / N, backend='nlp', W0=W0.T[None], h=p.time_step, keep_out=keep, **kw)
        ctx.sync()
        assert pl['entry'] == 'nlp_solve_keepout' and np.array_equal(pl['W'].cpu().numpy()[0], Wh) and pl['keep_mult'].shape == (1, 1, N)
