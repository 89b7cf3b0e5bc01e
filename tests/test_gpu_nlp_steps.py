"""GPU parity, Newton step by Newton step: the collocation solver (csrc/nlp_kernels.hip nlp_solve_one and what it calls -- nlp_assemble,
nlp_bcr / nlp_factor / nlp_backsolve, nlp_recover_stats, nlp_apply, nlp_merit) against its CPU statements after a BUDGET of steps
(d2d_nlp_opts.inner_max / outer_max), from the same start.

An end-of-solve comparison cannot see a wrong Newton step: the iteration corrects itself and reaches the same KKT point a few steps
later.  After k steps it can: the statement's early path is determined to 1e-14 .. 1e-11 (tests/test_nlp_steps_cpu.py), so the
iterates are compared to the tolerance tests/nlp_steps_ref.py measures on the statement alone, 1e3 x that floor -- four orders of
magnitude below the end-of-solve tolerances -- and the step count must be the statement's exactly: raises of the damping, halvings
of the line search and the progress gate are part of the path.

Budgets (inner_max, outer_max): (1,1) (2,1) (3,1) (5,1) (8,1), then (5,2) (5,3) (5,4), which cross the multiplier, penalty and barrier
updates.  After each: iters, all five planes of W, 2 rho mult against the statement's multipliers (tolerance x 2 rho), and cost / feas
against the statement's functions at the kernel's own W (1e-11 relative, 1e-12 absolute).

Entry points: d2d_nlp_solve (3 .. 129 nodes round the 64-node chunk, the 4-unroll and the 121-node LDS limit, cyclic reduction and
serial recursion; d2d_nlp_opts.bounds), d2d_nlp_solve_wind, d2d_nlp_solve_moving, d2d_nlp_solve_model (tests/nlp_model_ref.py),
and the group body: d2d_nlp_solve_groups, _groups_wind, _groups_pairs (constant wind and a field) and _groups_moving with 2 and 3
aircraft, one pair / a chain / all pairs coupled and 1 or 2 sweeps, every solve of the alternation under the budget; there W and the
summed step count of every aircraft, the sweeps and the last move are compared.

Measured on the run that added this module (MI355X), over all cases and budgets of an instantiation: the statement's floors, the
largest |W_kernel - W_statement| and the largest error / tolerance (the share of the 1e3 margin the kernel uses):
  plain (d2d_nlp_solve, 3 .. 129 nodes, both factorisations)  floors 4e-18 .. 8e-12   error 3.8e-11   error / tol 2.5e-02
  plain with d2d_nlp_opts.bounds (41 nodes)                   floors 5e-15 .. 3e-12   error 1.0e-11   error / tol 3.7e-03
  WIND (shear, vortex, gust; 41, 65, 122 nodes)               floors 7e-15 .. 6e-12   error 5.7e-12   error / tol 6.2e-03
  MOV (constant wind, 61 nodes)                               floors 2e-14 .. 8e-13   error 1.9e-11   error / tol 2.4e-01
  MOV + WIND (gust, 61 nodes)                                 floors 7e-15 .. 1e-11   error 2.6e-11   error / tol 2.4e-02
  MODEL (5, 41, 65 nodes; SPD, partial, indefinite)           floors 2e-16 .. 8e-12   error 1.9e-12   error / tol 1.8e-02
  d2d_nlp_solve_groups                                        floors 5e-15 .. 9e-12   error 2.7e-11   error / tol 9.7e-03
  d2d_nlp_solve_groups_wind                                   floors 5e-15 .. 7e-12   error 1.1e-12   error / tol 1.7e-02
  d2d_nlp_solve_groups_pairs, constant wind                   floors 5e-15 .. 9e-12   error 3.1e-11   error / tol 1.8e-02
  d2d_nlp_solve_groups_pairs, shear field                     floors 5e-15 .. 7e-12   error 3.8e-12   error / tol 3.7e-02
  d2d_nlp_solve_groups_moving                                 floors 5e-15 .. 9e-12   error 8.7e-11   error / tol 1.8e-02
Every step count, sweep count and multiplier agreed.  The full model solves: nodes within 2.4e-7 of the statement, KKT <= 2.3e-7.
Power of the comparison, same run: against a library built with the constraint-curvature entry D[3][4] of nlp_assemble dropped,
the first budget already fails -- 'plain-5-disc1 (1, 1): floor 7.1e-15, tol 7.1e-12: W off by 3.26e-01 at node 4, plane 4',
'plain-65-disc0 (1, 1): floor 1.0e-13, tol 1.0e-10: W off by 1.37e+00 at node 63, plane 4' -- while the end-of-solve tests
test_batch_with_obstacles_wind_and_boxes_vs_oracle, test_ragged_node_counts_vs_oracle (all seven) and
test_exp14_reproduces_the_reference_ipopt_cost still pass on it (test_costbank_max_mode_vs_oracle does notice it).
"""
import numpy as np
import pytest

import nlp_model_ref as MR
import nlp_moving_ref as M
import nlp_steps_ref as S
import nlp_wind_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def fields():
    return R.fields()


def _device_solve(ctx, fields, L, budget, W0=None, **kw):
    """One launch of L's entry point with the budget -> W (B, N, 5), out (numpy; mult as (B, N, 3))."""
    W = ctx.dev(np.ascontiguousarray(np.stack([c.W0[0].T for c in L.cases]) if W0 is None else W0))
    dsc = ctx.dev(np.ascontiguousarray(L.kw['rows']))
    if budget is not None:
        kw.update(inner_max=budget[0], outer_max=budget[1])
    F = fields[L.kw['field']] if L.kw.get('field') else None
    if L.entry == 'nlp_solve':
        b = L.kw.get('bounds')
        out = ctx.nlp_solve(dsc, W, S.H, want_mult=True, bounds=None if b is None else ctx.dev(np.ascontiguousarray(b)), **kw)
    elif L.entry == 'nlp_solve_wind':
        out = ctx.nlp_solve_wind(dsc, W, S.H, F, t_start=L.kw['t_start'], want_mult=True, **kw)
    elif L.entry == 'nlp_solve_moving':
        kn, dc = M.tables(L.kw['moving'])
        out = ctx.nlp_solve_moving(dsc, W, S.H, ctx.dev(kn), ctx.dev(dc), F, ctx.dev(np.ascontiguousarray(L.kw['t_start'])), want_mult=True, **kw)
    else:
        mps = L.kw['models']
        g = ctx.dev(np.ascontiguousarray(np.stack([m.g.T for m in mps])))
        Hp = ctx.dev(np.ascontiguousarray(np.stack([MR.pack(m.H) for m in mps])))
        Wc = ctx.dev(np.ascontiguousarray(np.stack([m.Wc.T for m in mps])))
        out = ctx.nlp_solve_model(dsc, W, S.H, g, Hp, Wc, want_mult=True, **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in ('cost', 'feas', 'iters', 'status', 'mult')}
    res['mult'] = res['mult'].transpose(0, 2, 1)
    return W.cpu().numpy().transpose(0, 2, 1), res


def _device_groups(ctx, fields, L, budget):
    """One launch of a groups entry point with the budget on every solve -> W (R, n_ac, N, 5), out (numpy)."""
    n_ac, N = L.kw['n_ac'], L.N
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for c in L.cases for w in c.W0])))
    dsc = ctx.dev(np.ascontiguousarray(L.kw['rows']))
    F = fields[L.kw['field']] if L.kw.get('field') else None
    t = ctx.dev(np.ascontiguousarray(L.kw['t_start']))
    kw = dict(max_sweeps=L.kw['max_sweeps'], inner_max=budget[0], outer_max=budget[1])
    if L.entry == 'nlp_solve_groups':
        out = ctx.nlp_solve_groups(dsc, W, S.H, n_ac, **kw)
    elif L.entry == 'nlp_solve_groups_wind':
        out = ctx.nlp_solve_groups_wind(dsc, W, S.H, n_ac, F, t, **kw)
    elif L.entry == 'nlp_solve_groups_pairs':
        out = ctx.nlp_solve_groups_pairs(dsc, W, S.H, n_ac, F, t if F is not None else None, **kw)
    else:
        kn, dc = M.tables(L.kw['moving'])
        out = ctx.nlp_solve_groups_moving(dsc, W, S.H, n_ac, ctx.dev(kn), ctx.dev(dc), F, t, **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in ('cost', 'feas', 'iters', 'status', 'sweeps', 'moved')}
    return W.cpu().numpy().transpose(0, 2, 1).reshape(len(L.cases), n_ac, N, 5), res


def _compare_groups(L, budget, W, out):
    """Every scenario of the launch against its statement: each aircraft's W and summed step count, the sweeps and the last move
    (a difference of two iterates: twice the tolerance)."""
    bad, worst, ratio = [], 0.0, 0.0
    n_ac = L.kw['n_ac']
    for r, case in enumerate(L.cases):
        m = S.measure(case, budget)
        info, tol = m['info'], m['tol']
        head = f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        its = tuple(int(i) for i in out['iters'][n_ac * r:n_ac * r + n_ac])
        if its != info['inner']:
            bad.append(f'{head}: iters {its}, the statement took {info["inner"]}')
        if int(out['sweeps'][r]) != info['sweeps']:
            bad.append(f'{head}: sweeps {out["sweeps"][r]}, the statement made {info["sweeps"]}')
        if not abs(out['moved'][r] - info['moved']) <= 2 * tol:
            bad.append(f'{head}: moved {out["moved"][r]!r}, the statement {info["moved"]!r}')
        for a in range(n_ac):
            dW = np.abs(W[r, a] - m['W'][a])
            err = float(dW.max())
            worst, ratio = max(worst, err), max(ratio, err / tol)
            if not err <= tol:
                i, c = np.unravel_index(np.argmax(dW), dW.shape)
                bad.append(f'{head}: aircraft {a}: W off by {err:.2e} at node {i}, plane {c}')
    return bad, worst, ratio


def _compare(L, budget, W, out, tag=''):
    """Every case of the launch against its statement after the budget -> list of complaints, largest error, largest error / tol."""
    bad, worst, ratio = [], 0.0, 0.0
    for b, case in enumerate(L.cases):
        m = S.measure(case, budget)
        info, tol = m['info']['raw'], m['tol']
        head = f'{case.cid}{tag} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        if int(out['iters'][b]) != info['inner']:
            bad.append(f'{head}: iters {out["iters"][b]}, the statement took {info["inner"]}')
        dW = np.abs(W[b] - m['W'][0])
        err = float(dW.max())
        worst, ratio = max(worst, err), max(ratio, err / tol)
        if not err <= tol:
            i, c = np.unravel_index(np.argmax(dW), dW.shape)
            bad.append(f'{head}: W off by {err:.2e} at node {i}, plane {c}')
        em = float(np.abs(2 * info['rho'] * out['mult'][b][1:] - info['mult']).max())
        if not em <= tol * 2 * info['rho']:
            bad.append(f'{head}: multipliers off by {em:.2e} > {tol * 2 * info["rho"]:.2e} (rho {info["rho"]:g})')
        cost, feas = case.fn(W[b])
        if not abs(out['cost'][b] - cost) <= 1e-11 * max(1.0, abs(cost)):
            bad.append(f'{head}: cost {out["cost"][b]!r}, the statement at the same W {cost!r}')
        if not abs(out['feas'][b] - feas) <= 1e-12:
            bad.append(f'{head}: feas {out["feas"][b]!r}, the statement at the same W {feas!r}')
    return bad, worst, ratio


@pytest.mark.parametrize('lid', S.launch_ids())
def test_kernel_follows_the_statement_step_by_step(ctx, fields, lid):
    L = S.launch(lid)
    bad, worst, ratio = [], 0.0, 0.0
    for serial in ((0, 1) if L.entry == 'nlp_solve' and 'bounds' not in L.kw else (0,)):
        for budget in S.BUDGETS:
            if 'groups' in L.entry:
                W, out = _device_groups(ctx, fields, L, budget)
                bd, w, r = _compare_groups(L, budget, W, out)
            else:
                W, out = _device_solve(ctx, fields, L, budget, serial=serial)
                bd, w, r = _compare(L, budget, W, out, ' serial' if serial else '')
            bad += bd; worst = max(worst, w); ratio = max(ratio, r)
    fl = [S.measure(c, b)['floor'] for c in L.cases for b in S.BUDGETS]
    print(f'{lid}: floors {min(fl):.1e} .. {max(fl):.1e}, largest |W - statement| {worst:.2e}, largest error / tol {ratio:.2e}')
    assert not bad, '\n'.join(bad)


def test_full_model_solves_vs_the_statement(ctx, fields):
    """One full solve per model (SPD, partial, indefinite) in one launch: verdicts equal, cost within 1e-7 relative and W within 1e-4
    of the statement (the end-of-solve tolerances of test_batch_with_obstacles_wind_and_boxes_vs_oracle), and the Lagrangian with the
    model's gradient g + H d stationary to 1e-5 at the kernel's point with the kernel's multipliers.  The bound duals in that residual
    are the statement's (the kernel keeps its own in its workspace and does not return them), as in the test named above: the
    stationarity check is the kernel's point and multipliers, not wholly its own KKT triple."""
    L = S.full_model_launch()
    W, out = _device_solve(ctx, fields, L, None)
    for b, (case, mp) in enumerate(zip(L.cases, L.kw['models'])):
        Wo, info = MR.solve(mp, case.W0[0])
        kkt, feas = MR.kkt_residual(mp, W[b], 2 * info['rho'] * out['mult'][b][1:], info['zL'], info['zU'])
        print(f'{case.cid}: status {out["status"][b]} / {info["status"]}, cost {out["cost"][b]:.12f} vs {info["cost"]:.12f}, '
              f'nodes {np.abs(W[b] - Wo).max():.2e}, steps {out["iters"][b]} / {info["inner"]}, kkt {kkt:.2e}')
        assert out['status'][b] == info['status'] == 1
        assert abs(out['cost'][b] - info['cost']) <= 1e-7 * max(abs(info['cost']), 1e-3)
        assert np.abs(W[b] - Wo).max() <= 1e-4
        assert abs(out['cost'][b] - mp.value(W[b])) <= 1e-11 * max(1.0, abs(out['cost'][b]))
        assert kkt <= 1e-5 and feas <= 1e-8, (kkt, feas)
