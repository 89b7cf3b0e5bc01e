"""GPU: the collocation solve outside hard keep-out discs that MOVE (include/d2d.h d2d_nlp_solve_keepout_moving, csrc/nlp_kernels.hip the
KMOV instantiations of nlp_solve_one) against its CPU statement tests/nlp_keepout_moving_ref.py.

Degenerate parity: tracks that stand still give the bytes of d2d_nlp_solve_keepout (W, cost, feas, iters, status, both sets of
multipliers) in constant wind and in the steady shear; no tracks give the bytes of d2d_nlp_solve.
Step by step: the method and the tolerance rule of tests/test_gpu_nlp_keepout.py / nlp_steps_ref, unchanged, at 3, 5, 17, 64, 65 and
121 nodes: a crossing disc, an overtaking disc and eight slots of which two are absent in one launch, the crossing disc in the steady
shear in a second one.  No case is skipped: tests/test_nlp_keepout_moving_cpu.py holds every one of them determined.
Full solves at 17, 41 and 121 nodes: status and step count equal the statement's, cost within 1e-7 relative and nodes within 1e-4 (the
bounds of tests/test_gpu_moving_obstacles.py), every g > 0, the continuous relative clearance at least the margin asked.
"""
import numpy as np
import pytest

import nlp_keepout_moving_ref as KM
import nlp_keepout_ref as K
import nlp_steps_ref as S
import nlp_wind_ref as R

pytestmark = pytest.mark.gpu
COST_RTOL, NODE_TOL = 1e-7, 1e-4


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    return ctx.dev(np.ascontiguousarray(a))


def mov_solve(ctx, rows, W0s, knots, disc, t_start, field=None, **kw):
    """One d2d_nlp_solve_keepout_moving launch: rows (B, stride), W0s B x (N, 5), knots (B, n, n_knot, 3), disc (B, n, 2) or None
    -> W (B, N, 5), out (numpy; mult (B, N, 3), keep_mult (B, n, N))."""
    W = _dev(ctx, np.stack([w.T for w in W0s]))
    out = ctx.nlp_solve_keepout_moving(_dev(ctx, rows), W, K.H0, None if knots is None else _dev(ctx, knots), None if disc is None else _dev(ctx, disc),
                                       field=field, t_start=t_start, want_mult=True, **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in ('cost', 'feas', 'iters', 'status', 'mult', 'keep_mult', 'mov_work') and v is not None}
    res['mult'] = res['mult'].transpose(0, 2, 1)
    return W.cpu().numpy().transpose(0, 2, 1), res


def _still(discs, n_knot=3):
    """static tables (B, n, 3) as tracks that stand still: knots (B, n, n_knot, 3), disc (B, n, 2)"""
    B, n, _ = discs.shape
    knots = np.zeros((B, n, n_knot, 3))
    knots[..., 0] = np.arange(n_knot) * 7.0 - 3.0
    knots[..., 1:] = discs[:, :, None, :2]
    disc = np.stack([discs[:, :, 2], np.ones((B, n))], -1)
    return knots, disc


@pytest.mark.parametrize('wind', ['const', 'shear'])
def test_tracks_that_stand_still_are_the_static_entry_bit_for_bit(ctx, wind):
    """The sampled centres are exact, and the KMOV instantiations pin the contraction of the discs' sums of two products to the static
    kernels' (csrc/nlp_kernels.hip nlp_dot2, nlp_keep_g; DESIGN.md 5.25 has what the other contraction costs)."""
    L = K.steps_launch(17)
    got = [L['shear']] if wind == 'shear' else [L[t] for t in K.STEP_TAGS if t != 'shear']
    got += K.full_launch(41) if wind == 'const' else []
    N = None
    for grp in ([g for g in got if len(g) == 4], [g for g in got if len(g) == 5]):
        if not grp:
            continue
        if len(grp[0]) == 4:
            rows, W0s, discs = np.stack([g[1] for g in grp]), [g[0].W0[0][:17] for g in grp], np.stack([g[2] for g in grp])
        else:
            rows, W0s, discs = np.stack([g[1] for g in grp]), [g[2] for g in grp], np.stack([g[3] for g in grp])
        field, t0 = (R.fields()['shear'], 0.75) if wind == 'shear' else (None, 0.75)
        Wd = _dev(ctx, np.stack([w.T for w in W0s]))
        st = ctx.nlp_solve_keepout(_dev(ctx, rows), Wd, K.H0, _dev(ctx, discs), field=field, t_start=t0 if field is not None else None, want_mult=True)
        ctx.sync()
        W, out = mov_solve(ctx, rows, W0s, *_still(discs), t0, field)
        Wst = Wd.cpu().numpy().transpose(0, 2, 1)
        print(f'{wind}-{W.shape[1]}: largest |W - static W| {np.abs(W - Wst).max():.2e}, iters {out["iters"].tolist()} / {st["iters"].cpu().numpy().tolist()}, '
              f'largest |z - static z| {np.abs(out["keep_mult"] - st["keep_mult"].cpu().numpy()).max():.2e}, '
              f'centres exact: {all((out["mov_work"][b, m].T == discs[b, m, :2]).all() for b in range(len(discs)) for m in range(discs.shape[1]))}')
        assert W.tobytes() == Wst.tobytes()
        for k in ('cost', 'feas', 'iters', 'status', 'keep_mult'):
            assert out[k].tobytes() == st[k].cpu().numpy().tobytes(), k
        assert out['mult'].tobytes() == st['mult'].cpu().numpy().transpose(0, 2, 1).tobytes()
        assert (out['status'] != 3).all() and out['iters'].min() > 5 and out['keep_mult'].any()      # (solved, not refused alike)
        N = W.shape[1]
    assert N is not None


def test_no_tracks_is_the_plain_solve_bit_for_bit(ctx):
    got = [S.plain_case(41, tag, 0) for tag in ('disc1', 'windbox')]
    rows, W0s = np.stack([g[1] for g in got]), [g[0].W0[0] for g in got]
    Wk, ok = mov_solve(ctx, rows, W0s, None, None, None)
    Wd = _dev(ctx, np.stack([w.T for w in W0s]))
    op = ctx.nlp_solve(_dev(ctx, rows), Wd, K.H0)
    ctx.sync()
    assert Wk.tobytes() == Wd.cpu().numpy().transpose(0, 2, 1).tobytes() and (ok['status'] == 1).all()
    for k in ('cost', 'feas', 'iters', 'status'):
        assert ok[k].tobytes() == op[k].cpu().numpy().tobytes(), k
    assert 'keep_mult' not in ok


def _compare(cases, budget, W, out):
    bad, worst, ratio = [], 0.0, 0.0
    for b, case in enumerate(cases):
        m = S.measure(case, budget)
        info, tol = m['info']['raw'], m['tol']
        head = f'{case.cid} {budget}: floor {m["floor"]:.1e}, tol {tol:.1e}'
        assert tol <= S.TOL_CAP, head                       # (no case is skipped as undetermined: the CPU module holds them all)
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


@pytest.mark.parametrize('N', KM.STEP_N)
def test_kernel_follows_the_statement_step_by_step(ctx, N):
    L = KM.steps_launch(N)
    const = [L[t] for t in KM.STEP_TAGS if t != 'shear']
    groups = [(const, None), ([L['shear']], R.fields()[KM.STEP_FIELD])]
    bad, worst, ratio = [], 0.0, 0.0
    for budget in S.BUDGETS:
        for got, field in groups:
            cases = [g[0] for g in got]
            knots, disc = KM.tables([g[2] for g in got])
            W, out = mov_solve(ctx, np.stack([g[1] for g in got]), [c.W0[0][:N] for c in cases], knots, disc, KM.STEP_T_START, field,
                               inner_max=budget[0], outer_max=budget[1])
            bd, w, r = _compare(cases, budget, W, out)
            bad += bd; worst = max(worst, w); ratio = max(ratio, r)
    fl = [S.measure(g[0], b)['floor'] for g in L.values() for b in S.BUDGETS]
    print(f'keepmov-{N}: floors {min(fl):.1e} .. {max(fl):.1e}, largest |(W, z) - statement| {worst:.2e}, largest error / tol {ratio:.2e}')
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('N', KM.FULL_N)
def test_full_solves_vs_the_statement(ctx, N):
    import d2d.opty_utils as ou
    got = KM.full_launch(N)
    rows, W0s = np.stack([g[1] for g in got]), [g[2] for g in got]
    knots, disc = KM.tables([g[3] for g in got])
    W, out = mov_solve(ctx, rows, W0s, knots, disc, KM.FULL_T_START)
    t = KM.FULL_T_START + np.arange(N) * K.H0
    for b, (prob, _, W0, trs, ko) in enumerate(got):
        Wr, info = KM.solve_moving(prob.pb, W0, trs, KM.FULL_T_START)
        ctr, Rr = KM.centres(trs, KM.FULL_T_START, N, K.H0)
        gk = KM.g_values(W[b][1:-1], ctr[:, 1:-1], Rr)[0]
        dctr = float(np.abs(out['mov_work'][b, 0].T - ctr[0]).max())
        cl = ou.moving_keep_clearance([ko], t, W[b][:, 0], W[b][:, 1])[0]
        dn = float(np.abs(W[b] - Wr).max())
        print(f'{N}-{b}: status {out["status"][b]} / {info["status"]}, steps {out["iters"][b]} / {info["inner"]}, cost {out["cost"][b]:.12f} vs {info["cost"]:.12f}, '
              f'nodes off by {dn:.2e}, feas {out["feas"][b]:.1e}, min g {gk.min():.2e}, centres off by {dctr:.1e}, clearance {cl:.4f} (margin {ko.margin:.4f})')
        assert out['status'][b] == info['status'] == 1 and out['iters'][b] == info['inner']
        assert abs(out['cost'][b] - info['cost']) <= COST_RTOL * max(info['cost'], 1e-3) and dn <= NODE_TOL
        assert out['feas'][b] <= 1e-9 and gk.min() > 0.0 and dctr <= 1e-12
        assert gk.min() / Rr[0] ** 2 < 1e-6 and out['keep_mult'][b][0].max() > 0.0                 # the disc binds
        assert not out['keep_mult'][b][:, [0, -1]].any() and not out['keep_mult'][b][1:].any()     # end nodes and absent slots
        assert cl >= ko.margin


def test_against_the_slsqp_arbiter(ctx):
    """The kernel against scipy SLSQP with the node inequalities as true constraints (tests/golden/nlp_keepout_moving_slsqp.npz: 5, 9,
    17 nodes, a crossing and an overtaking disc): the cost to tests/test_nlp_keepout_moving_cpu.py's tolerance, 10 x the largest
    difference measured on the statement when the file was made."""
    from test_nlp_keepout_moving_cpu import SLSQP_COST_RTOL, golden_cases
    n = 0
    for k, pb, row, W0, trs, t0, cost in golden_cases():
        knots, disc = KM.tables([trs])
        W, out = mov_solve(ctx, row[None], [W0], knots, disc, t0)
        ctr, Rr = KM.centres(trs, t0, pb.N, pb.h)
        gk = KM.g_values(W[0][1:-1], ctr[:, 1:-1], Rr)[0]
        dc = abs(out['cost'][0] - cost) / cost
        n += 1
        print(f'case {k} (N {pb.N}): status {out["status"][0]}, cost off by {dc:.2e} relative, feas {out["feas"][0]:.1e}, min g {gk.min():.1e}')
        assert out['status'][0] == 1 and out['feas'][0] <= 1e-9 and gk.min() >= 0.0
        assert dc <= SLSQP_COST_RTOL
    assert n == 6


def test_device_refusals(ctx):
    """Six problems in one launch: a NaN knot, knot times that do not increase, a NaN t_start, a NaN R, an end pose inside the disc at
    node N - 1's time whose static disc at the first knot would be accepted, and a good problem, which is solved."""
    import d2dhip
    N = 41
    prob, r, W0, trs, ko = KM.full_launch(N)[0]
    pb = prob.pb
    good_k, good_d = KM.tables([trs])
    knots, disc = np.repeat(good_k, 6, 0), np.repeat(good_d, 6, 0)
    t_start = np.full(6, KM.FULL_T_START)
    knots[0, 0, 1, 1] = np.nan
    knots[1, 0, 1, 0] = knots[1, 0, 0, 0]
    t_start[2] = np.nan
    disc[3, 4, 0] = np.nan                                   # (a slot behind the live one)
    T = (N - 1) * K.H0
    far = pb.p1[:2] + np.array([0.0, 10.0 * trs[0].r])
    arrive = KM.Track((KM.FULL_T_START, KM.FULL_T_START + T), (far, pb.p1[:2] + 0.2 * trs[0].r), trs[0].r)
    knots[4], disc[4] = KM.tables([[arrive]])[0][0], KM.tables([[arrive]])[1][0]
    W, out = mov_solve(ctx, np.stack([r] * 6), [W0] * 6, knots, disc, ctx.dev(t_start))
    print(f'status {out["status"].tolist()}, cost {out["cost"].tolist()}')
    for b in range(5):
        assert out['status'][b] == d2dhip.ST_NONFINITE and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and out['iters'][b] == 0, b
        assert W[b].tobytes() == W0.tobytes(), b
    # the static entry accepts the disc of problem 4 where its first knot puts it; the statement refuses the moving one
    st = ctx.nlp_solve_keepout(_dev(ctx, r[None]), _dev(ctx, W0.T[None]), K.H0, _dev(ctx, np.array([[[far[0], far[1], trs[0].r]]])))
    ctx.sync()
    assert int(st['status'][0].item()) == 1
    assert KM.solve_moving(pb, W0, [arrive], KM.FULL_T_START)[1]['status'] == KM.ST_NONFINITE
    _, info = KM.solve_moving(pb, W0, trs, KM.FULL_T_START)
    assert out['status'][5] == info['status'] == 1 and out['iters'][5] == info['inner']
    assert abs(out['cost'][5] - info['cost']) <= COST_RTOL * max(info['cost'], 1e-3)
    with pytest.raises(d2dhip.D2DError, match=r'error -1: .*t_start'):                   # D2D_EINVAL: tracks without a start time
        mov_solve(ctx, r[None], [W0], good_k, good_d, None)


def test_order_only_schedules(ctx):
    import torch
    got = KM.full_launch(41)
    rows, W0s = np.stack([g[1] for g in got] * 3), [g[2] for g in got] * 3
    knots, disc = KM.tables([g[3] for g in got] * 3)
    W, out = mov_solve(ctx, rows, W0s, knots, disc, KM.FULL_T_START)
    order = torch.tensor([5, 3, 1, 0, 2, 4], dtype=torch.int32, device=ctx.device)
    Wo, oo = mov_solve(ctx, rows, W0s, knots, disc, KM.FULL_T_START, order=order, slots=2)
    assert W.tobytes() == Wo.tobytes() and (out['status'] == 1).all()
    for k in ('cost', 'feas', 'iters', 'status', 'keep_mult', 'mult'):
        assert out[k].tobytes() == oo[k].tobytes(), k


def test_nlp_plan_routes_to_the_entry(ctx):
    import d2dhip
    prob, r, W0, trs, ko = KM.full_launch(41)[0]
    knots, disc = KM.tables([trs])
    W, out = mov_solve(ctx, r[None], [W0], knots, disc, KM.FULL_T_START)
    Wd = _dev(ctx, W0.T[None])
    pl = d2dhip.nlp_plan(ctx, _dev(ctx, r[None]), Wd, K.H0, hard_knots=_dev(ctx, knots), hard_disc=_dev(ctx, disc), t_start=KM.FULL_T_START)
    ctx.sync()
    assert pl['entry'] == 'nlp_solve_keepout_moving' and Wd.cpu().numpy().transpose(0, 2, 1).tobytes() == W.tobytes()
    assert pl['keep_mult'].shape == (1, KM.MAX_MOV, 41)


def test_planner_routes_a_moving_keep_out_to_the_entry(ctx):
    """single_opt_planner.Planner on exp_14 with a MovingKeepOut across its free plan, in constant wind and in a field: the plan of
    Context.nlp_solve_keepout_moving on the same row, start and lowered tables; info['keep_out_clearance'] is the continuous clearance
    against the moving centre, per disc, and holds the margin where the plan without the disc does not."""
    import d2d.optyplan_scenarios as sc
    import d2d.opty_utils as ou
    import single_opt_planner as sop
    from test_nlp_keepout_cpu import _exp14
    from test_nlp_keepout_moving_cpu import moving_disc_across
    mk = moving_disc_across(sc.exp_14)
    far = ou.KeepOut((40.0, 40.0), 2.0)
    for wf in (None, -R.fields()['shear']):                  # (the planner's convention: a plan for a plant that flies F is solved in -F)
        attrs = dict(keep_out=[mk, far], **({} if wf is None else dict(wind=wf)))
        p = sop.Planner(_exp14(**attrs), backend='auto')
        x0 = p.get_initial_guess()
        p.run(x0)
        assert p.info['backend_used'] == 'nlp' and p.info['status'] == 1, p.info
        cl = p.info['keep_out_clearance']
        t = p.prob.t_start + np.arange(p.num_nodes) * p.time_step
        print(f'exp_14 round {mk} ({"constant wind" if wf is None else "shear"}): clearance {cl}, cost {p.info["obj_val"]:.9f}, steps {p.info["iters"]}')
        assert len(cl) == 2 and cl[0] >= mk.margin and cl[1] > 10.0
        assert cl == ou.moving_keep_clearance([mk, far], t, p.sol_x, p.sol_y)
        q = sop.Planner(_exp14(**{k: v for k, v in attrs.items() if k != 'keep_out'}), backend='nlp'); q.run(q.get_initial_guess())
        clq = ou.moving_keep_clearance([mk], t, q.sol_x, q.sol_y)[0]
        print(f'  without the disc: clearance {clq:.4f}')
        assert 'keep_out_clearance' not in q.info and (wf is not None or clq < mk.margin)       # (the disc was laid across the constant-wind plan)
        # the direct solve
        rows, _ = p.prob._rows()
        W0 = np.stack([x0[s] for s in (p._slice_x, p._slice_y, p._slice_psi, p._slice_phi, p._slice_v)], 1)
        W = _dev(ctx, W0.T[None])
        out = ctx.nlp_solve_keepout_moving(ctx.dev(rows), W, p.time_step, ctx.dev(p.prob.keep_knots[None]), ctx.dev(p.prob.keep_disc[None]),
                                           field=p.prob.field, t_start=p.prob.t_start, **p.prob._solver_kw())
        ctx.sync()
        Wh = W.cpu().numpy()[0]
        assert int(out['status'][0].item()) == 1
        assert np.array_equal(Wh[0], p.sol_x) and np.array_equal(Wh[1], p.sol_y) and np.array_equal(Wh[4], p.sol_v)
