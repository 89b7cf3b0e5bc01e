"""GPU: the collocation solve with a free time step (include/d2d.h d2d_nlp_solve_free, csrc/nlp_kernels.hip FREE instantiation of
nlp_solve_one: nlp_assemble's border, the two passes of nlp_bcr, nlp_recover_free, nlp_merit at the trial step) against its CPU
statement tests/nlp_free_ref.py and against the SLSQP arbiter tests/golden/nlp_free_slsqp.npz.

Step by step, on the method of tests/test_gpu_nlp_steps.py: after each budget (inner_max, outer_max) of nlp_steps_ref.BUDGETS the step
count must be the statement's exactly, and W, h (and u = 1 / h) and 2 rho mult must lie within 1e3 x the floor that the statement
shows against itself when every entry of its start moves by an ulp (nlp_steps_ref.measure on the iterate with its interval,
nlp_free_ref.ext).  Node counts 3, 5, 17, 64, 65, 121, 122, 129 (one free node; the chunk edge; the LDS limit of the cyclic reduction; a
ragged last chunk), each a launch of a kind-1 disc with k_dur = 0.5, a kind-0 disc with k_dur = 0 and a y box in constant wind with
k_dur = 2; and a 41-node launch with d2d_nlp_opts.bounds, the same row without, and the same row with h_lo 5 % above its own interior
optimum, whose h ends on that bound.

Measured on the run that added this module (MI355X), per launch over its cases and the eight budgets: the statement's floors, the largest
|(W, h, u)_kernel - statement| and the largest error / tolerance (the share of the 1e3 margin the kernel uses):
  3 nodes        floors 6.9e-18 .. 8.9e-15   error 4.3e-15   error / tol 1.4e-02
  5 nodes        floors 1.1e-16 .. 1.4e-14   error 3.7e-15   error / tol 1.0e-02
  17 nodes       floors 1.8e-15 .. 4.7e-12   error 5.1e-13   error / tol 9.0e-03
  64 nodes       floors 2.5e-14 .. 3.9e-12   error 2.2e-12   error / tol 1.8e-03
  65 nodes       floors 3.2e-14 .. 8.5e-12   error 5.7e-12   error / tol 8.9e-04
  121 nodes      floors 7.3e-14 .. 9.4e-12   error 1.9e-12   error / tol 1.1e-02
  122 nodes      floors 5.7e-14 .. 7.7e-12   error 1.2e-12   error / tol 6.4e-04
  129 nodes      floors 8.3e-14 .. 6.6e-12   error 3.1e-12   error / tol 5.4e-03
  bounds (41)    floors 3.6e-15 .. 3.6e-12   error 1.7e-12   error / tol 5.7e-04   (h of the third case: 0.10039849009560, h_lo 0.10039849006971)
Every step count and multiplier agreed.
Power of the comparison, same run: against a library built with the cross-curvature term of the border dropped (rho (c + mu) on
b, both signs; local build, not committed) the first budget already fails:
  'free-17-disc1 (1, 1): floor 1.1e-14, tol 1.1e-11: W off by 3.34e-02 at node 17, plane 1 (the row of h, u)'
  'free-17-disc0 (5, 1): floor 1.6e-14, tol 1.6e-11: W off by 3.44e-02 at node 7, plane 4'
and every later budget with them (largest error / tol 1.1e+10), while that build still converges on the full solves.
"""
import os

import numpy as np
import pytest

import nlp_free_ref as F
import nlp_steps_ref as S
from oracle import nlp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nlp_free_slsqp.npz')
COST_RTOL = 1e-7                 # tests/test_gpu_nlp.py: |cost - statement's| <= 1e-7 max(cost, 1e-3) at the end of a solve


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def free_solve(ctx, rows, W0s, fr, bounds=None, h0=F.H0, **kw):
    """One d2d_nlp_solve_free launch: rows (B, stride), W0s (B, N, 5), fr (B, 4) -> W (B, N, 5), out (numpy; mult (B, N, 3))."""
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    out = ctx.nlp_solve_free(ctx.dev(np.ascontiguousarray(rows)), W, h0, ctx.dev(np.ascontiguousarray(fr)), want_mult=True,
                             bounds=None if bounds is None else ctx.dev(np.ascontiguousarray(bounds)), **kw)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items() if k in ('cost', 'feas', 'iters', 'status', 'mult', 'h')}
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
        We = np.concatenate([W[b], [[out['h'][b], 1.0 / out['h'][b], 0.0, 0.0, 0.0]]])
        dW = np.abs(We - m['W'][0])
        err = float(dW.max())
        worst, ratio = max(worst, err), max(ratio, err / tol)
        if not err <= tol:
            i, c = np.unravel_index(np.argmax(dW), dW.shape)
            bad.append(f'{head}: W off by {err:.2e} at node {i}, plane {c}' + (' (the row of h, u)' if i == W[b].shape[0] else ''))
        em = float(np.abs(2 * info['rho'] * out['mult'][b][1:] - info['mult']).max())
        if not em <= tol * 2 * info['rho']:
            bad.append(f'{head}: multipliers off by {em:.2e} > {tol * 2 * info["rho"]:.2e} (rho {info["rho"]:g})')
        cost, feas = case.fn(W[b], out['h'][b])
        if not abs(out['cost'][b] - cost) <= 1e-11 * max(1.0, abs(cost)):
            bad.append(f'{head}: cost {out["cost"][b]!r}, the statement at the same W, h {cost!r}')
        if not abs(out['feas'][b] - feas) <= 1e-12 * max(1.0, 1.0 / out['h'][b]):
            bad.append(f'{head}: feas {out["feas"][b]!r}, the statement at the same W, h {feas!r}')
    return bad, worst, ratio


@pytest.mark.parametrize('lid', [str(N) for N in F.STEP_N] + ['bounds'])
def test_kernel_follows_the_statement_step_by_step(ctx, lid):
    cases, rows, fr, bnd = F.bounds_launch() if lid == 'bounds' else F.steps_launch(int(lid))
    bad, worst, ratio = [], 0.0, 0.0
    for budget in S.BUDGETS:
        W, out = free_solve(ctx, rows, [c.W0[0][:-1] for c in cases], fr, bnd, inner_max=budget[0], outer_max=budget[1])
        bd, w, r = _compare(cases, budget, W, out)
        bad += bd; worst = max(worst, w); ratio = max(ratio, r)
    fl = [S.measure(c, b)['floor'] for c in cases for b in S.BUDGETS]
    print(f'free-{lid}: floors {min(fl):.1e} .. {max(fl):.1e}, largest |(W, h) - statement| {worst:.2e}, largest error / tol {ratio:.2e}')
    if lid == 'bounds':                      # the third case ends on its lower bound: a full solve puts h within 1e-6 relative of h_lo
        W, out = free_solve(ctx, rows, [c.W0[0][:-1] for c in cases], fr, bnd)
        print(f'free-bounds-hlo: h {out["h"][2]!r}, h_lo {fr[2, 0]!r}, status {out["status"][2]}')
        assert out['status'][2] == 1 and fr[2, 0] < out['h'][2] <= fr[2, 0] * (1 + 1e-6)
    assert not bad, '\n'.join(bad)


FULL = {17: [(s, kw) for s in (0, 1) for kw in (dict(k_dur=0.5), dict(k_dur=0.5, obstacle=1), dict(k_dur=2.0), dict(k_dur=1.0, obstacle=0))],
        41: [(s, kw) for s in (0, 1) for kw in (dict(k_dur=0.5), dict(k_dur=0.5, obstacle=1), dict(k_dur=2.0), dict(k_dur=1.0, obstacle=0))],
        121: [(s, kw) for s in (0, 1) for kw in (dict(k_dur=0.5), dict(k_dur=0.5, obstacle=1), dict(k_dur=2.0), dict(k_dur=1.0, obstacle=0))]}


@pytest.mark.parametrize('N', sorted(FULL))
def test_full_solves_vs_the_statement(ctx, N):
    """Eight full solves per node count in one launch: the statement's verdict, cost and h to the end-of-solve tolerance of
    tests/test_gpu_nlp.py, feas <= 1e-9, h strictly inside its box.  (Node values are not compared: they are not unique in the flat
    directions of the objective.)"""
    got = [F.leg_problem(N, 300 + s, **kw) for s, kw in FULL[N]]
    fr = F.free_rows([g[0] for g in got])
    W, out = free_solve(ctx, np.stack([g[1] for g in got]), [g[2] for g in got], fr)
    for b, (fp, _, W0) in enumerate(got):
        _, info = F.solve(fp, W0, F.H0)
        print(f'{N}-{b}: status {out["status"][b]} / {info["status"]}, cost {out["cost"][b]:.12f} vs {info["cost"]:.12f}, h {out["h"][b]:.12f} vs {info["h"]:.12f}, '
              f'steps {out["iters"][b]} / {info["inner"]}, feas {out["feas"][b]:.1e}')
        assert out['status'][b] == info['status'] == 1
        assert abs(out['cost'][b] - info['cost']) <= COST_RTOL * max(info['cost'], 1e-3)
        assert abs(out['h'][b] - info['h']) <= COST_RTOL * max(info['h'], 1e-3)
        assert out['feas'][b] <= 1e-9 and fp.h_lo < out['h'][b] < fp.h_hi
        assert abs(out['cost'][b] - fp.cost(W[b], 1.0 / out['h'][b])) <= 1e-11 * max(1.0, out['cost'][b])


def test_against_the_slsqp_arbiter(ctx):
    """The kernel against scipy SLSQP on the same problems with h itself as a variable (5, 9, 17 nodes): cost and h to
    tests/test_nlp_free_cpu.py's tolerance, measured there on the statement: 10 x its largest difference over these cases."""
    from test_nlp_free_cpu import SLSQP_COST_RTOL, SLSQP_H_RTOL
    g = np.load(GOLDEN)
    for k in range(int(g['n_cases'])):
        N = int(g[f'c{k}_N'])
        W, out = free_solve(ctx, g[f'c{k}_row'][None], [g[f'c{k}_W0']], g[f'c{k}_free_row'][None])
        dc, dh = abs(out['cost'][0] - g[f'c{k}_cost']) / g[f'c{k}_cost'], abs(out['h'][0] - g[f'c{k}_h']) / g[f'c{k}_h']
        print(f'case {k} (N {N}): status {out["status"][0]}, cost off by {dc:.2e} relative, h by {dh:.2e} relative, feas {out["feas"][0]:.1e}')
        assert out['status'][0] == 1 and out['feas'][0] <= 1e-9
        assert dc <= SLSQP_COST_RTOL and dh <= SLSQP_H_RTOL


def test_fixed_step_solve_agrees_at_the_solved_step(ctx):
    """d2d_nlp_solve with h fixed at h_out, started from the free solution's W, converges, and its cost is the free solve's minus the
    duration term.  Tolerance: 10 x what the two CPU statements (tests/nlp_free_ref.py, then oracle.nlp at its h from its W) show for
    the same four pairs -- measured 4.6e-10, 4.2e-8, 2.9e-10, 5.8e-11 relative: the fixed-step solve starts from a point that is
    stationary to opt_tol and takes a few more steps.  (The kernels showed the same four figures.)"""
    N = 41
    got = [F.leg_problem(N, 300 + s, **kw) for s, kw in FULL[N][:4]]
    fr = F.free_rows([g[0] for g in got])
    rows = np.stack([g[1] for g in got])
    W, out = free_solve(ctx, rows, [g[2] for g in got], fr)
    worst = 0.0
    for b, (fp, _, W0) in enumerate(got):
        assert out['status'][b] == 1
        Wd = ctx.dev(np.ascontiguousarray(W[b].T[None]))
        o2 = ctx.nlp_solve(ctx.dev(rows[b][None]), Wd, float(out['h'][b]))
        ctx.sync()
        c2, s2 = float(o2['cost'][0].item()), int(o2['status'][0].item())
        want = out['cost'][b] - fp.k_dur * (N - 1) * out['h'][b]
        # the two CPU statements on the same pair
        Ws, info = F.solve(fp, W0, F.H0)
        _, i2 = nlp.solve(fp.at(info['u']), Ws)
        ref = abs(i2['cost'] - (info['cost'] - fp.k_dur * (N - 1) * info['h'])) / max(i2['cost'], 1e-3)
        d = abs(c2 - want) / max(want, 1e-3)
        worst = max(worst, d)
        print(f'{b}: fixed-step status {s2}, cost {c2:.12f} vs free - duration {want:.12f}: off by {d:.2e} relative (the statements: {ref:.2e})')
        assert s2 == 1 and i2['status'] == 1
        assert d <= FIXED_VS_FREE
    print(f'largest {worst:.2e}')


FIXED_VS_FREE = 4.2e-7


def test_refusals_in_a_mixed_batch(ctx):
    """Rows with h_lo <= 0, h_lo >= h_hi, NaN and k_dur < 0 among good rows: ST_NONFINITE, NaN cost, W bit-identical to the input; the
    good rows bit-identical to a batch without the bad ones."""
    N = 41
    got = [F.leg_problem(N, 300 + s, **kw) for s, kw in FULL[N][:4]]
    good_fr = F.free_rows([g[0] for g in got])
    badrows = [(0.0, 0.2, 0.5, 0.0), (-0.05, 0.2, 0.5, 0.0), (0.2, 0.2, 0.5, 0.0), (0.3, 0.2, 0.5, 0.0), (np.nan, 0.2, 0.5, 0.0),
               (0.05, np.inf, 0.5, 0.0), (0.05, 0.2, -1.0, 0.0), (0.05, 0.2, 0.5, np.nan), (0.05, 0.2, 0.5, np.inf)]
    rows, W0s, fr, is_bad = [], [], [], []
    for k in range(len(badrows) + len(got)):
        if k % 3 == 1 and len([x for x in is_bad if not x]) < len(got):
            j = len([x for x in is_bad if not x])
            rows.append(got[j][1]); W0s.append(got[j][2]); fr.append(good_fr[j]); is_bad.append(False)
        elif len([x for x in is_bad if x]) < len(badrows):
            j = len([x for x in is_bad if x])
            rows.append(got[j % 4][1]); W0s.append(got[j % 4][2]); fr.append(badrows[j]); is_bad.append(True)
        else:
            j = len([x for x in is_bad if not x])
            rows.append(got[j][1]); W0s.append(got[j][2]); fr.append(good_fr[j]); is_bad.append(False)
    is_bad = np.array(is_bad)
    assert is_bad.sum() == len(badrows) and (~is_bad).sum() == len(got)
    W, out = free_solve(ctx, np.stack(rows), W0s, np.array(fr))
    Wg, og = free_solve(ctx, np.stack([g[1] for g in got]), [g[2] for g in got], good_fr)
    for b in np.flatnonzero(is_bad):
        assert out['status'][b] == 3 and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and np.isnan(out['h'][b]) and out['iters'][b] == 0, (b, fr[b])
        assert np.array_equal(W[b], W0s[b]), b
    gi = np.flatnonzero(~is_bad)
    assert (og['status'] == 1).all()
    assert np.array_equal(W[gi], Wg)
    for k in ('cost', 'feas', 'h', 'iters', 'status', 'mult'):
        assert np.array_equal(out[k][gi], og[k]), k


def test_order_only_schedules(ctx):
    """B = 64 problems of 41 nodes: a reversed hand-out order gives bit-identical W, h, cost, iters and status."""
    import torch
    N, B = 41, 64
    got = [F.leg_problem(N, 400 + b, k_dur=0.5 + 0.1 * (b % 5), obstacle=(None, 1, 0)[b % 3]) for b in range(B)]
    fr = F.free_rows([g[0] for g in got])
    rows = np.stack([g[1] for g in got])
    W1, o1 = free_solve(ctx, rows, [g[2] for g in got], fr)
    order = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=ctx.device).contiguous()
    W2, o2 = free_solve(ctx, rows, [g[2] for g in got], fr, order=order)
    assert (o1['status'] == 1).sum() >= B // 2, o1['status']
    assert np.array_equal(W1, W2)
    for k in ('cost', 'feas', 'h', 'iters', 'status'):
        assert np.array_equal(o1[k], o2[k], equal_nan=True), k


def _exp13(free):
    import d2d.optyplan_scenarios as sc
    return type('exp_13_free', (sc.exp_13,), {'t1_free': (2.0, 6.0)}) if free else sc.exp_13


def test_exp13_through_the_planner(ctx, tmp_path):
    """exp_13 with t1_free = (2.0, 6.0): CONVERGED, duration >= 3.3 s (the analytic bound of DESIGN.md 5.8), sol_time follows, bounds
    held; without t1_free it stays STALLED; Problem(time_step=Symbol) returns the same plan with the interval as the last entry."""
    import sympy
    import opty.direct_collocation as odc
    import single_opt_planner as sop
    e = _exp13(True)
    p = sop.Planner(e)
    p.run()
    print(f'exp_13 free: status {p.info["status"]}, duration {p.duration!r}, time_step {p.time_step!r}, cost {p.info["obj_val"]!r}, feas {p.info["feas"]:.1e}')
    assert p.info['status'] == 1 and p.info['backend_used'] == 'nlp'
    assert p.duration >= 3.3 and p.sol_time[-1] == p.duration and p.info['duration'] == p.duration and p.info['time_step'] == p.time_step
    assert 2.0 < p.duration < 6.0 and p.info['feas'] <= 1e-9
    assert e.phi_constraint[0] <= p.sol_phi.min() and p.sol_phi.max() <= e.phi_constraint[1]
    assert e.v_constraint[0] <= p.sol_v.min() and p.sol_v.max() <= e.v_constraint[1]
    assert (p.sol_x[0], p.sol_y[0], p.sol_x[-1], p.sol_y[-1]) == (e.p0[0], e.p0[1], e.p1[0], e.p1[1])
    p.save_solution(str(tmp_path / 'exp13_free.npz'))
    saved = np.load(str(tmp_path / 'exp13_free.npz'))
    assert saved['sol_time'][-1] == p.duration and float(saved['time_step']) == p.time_step and float(saved['duration']) == p.duration
    q = sop.Planner(_exp13(False), backend='nlp')
    q.run()
    assert q.info['status'] == 4, q.info['status']
    # the same Problem spelled as upstream opty does: a sympy Symbol for the interval, its bound in `bounds`
    h = sympy.Symbol('h')
    g, cost = q.aircraft, e.cost
    bounds = {g._sphi(g._st): e.phi_constraint, g._sv(g._st): e.v_constraint, h: (2.0 / 30, 6.0 / 30)}
    prob = odc.Problem(lambda f: cost.cost(f, q), lambda f: cost.cost_grad(f, q), g.get_eom(e.wind), g._state_symbols, 31, h,
                       known_parameter_map={}, instance_constraints=q._instance_constraints, bounds=bounds)
    assert prob.num_free == 5 * 31 + 1
    sol, info = prob.solve(np.concatenate([q.get_initial_guess(), [0.1]]))
    assert info['status'] == 1 and np.array_equal(sol, p.solution) and sol[-1] == p.time_step


def test_plan_batch_free_time_matches_a_direct_solve(ctx):
    import full_sim
    N = 41
    got = [F.leg_problem(N, 300 + s, **kw) for s, kw in FULL[N][:4]]
    rows = np.stack([g[1] for g in got])
    W0 = np.ascontiguousarray(np.stack([g[2].T for g in got]))
    kd = np.array([g[0].k_dur for g in got])
    out = full_sim.plan_batch(rows, N, (N - 1) * F.H0, 1.0 / N, backend='nlp', W0=W0, h=F.H0, free_time=(0.05, 0.2), kdur=kd)
    W, ref = free_solve(ctx, rows, [g[2] for g in got], F.free_rows([g[0] for g in got]))
    ctx.sync()
    assert np.array_equal(out['h'].cpu().numpy(), ref['h']) and np.array_equal(out['cost'].cpu().numpy(), ref['cost'])
    assert np.array_equal(out['W'].cpu().numpy().transpose(0, 2, 1), W) and (ref['status'] == 1).all()
    with pytest.raises(NotImplementedError, match='n_ac > 1'):
        full_sim.plan_batch(rows, N, (N - 1) * F.H0, 1.0 / N, backend='nlp', W0=W0, h=F.H0, n_ac=2, free_time=(0.05, 0.2))
