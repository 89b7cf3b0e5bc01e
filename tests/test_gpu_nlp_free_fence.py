"""GPU: the collocation solve with a free time step outside static hard discs and inside a convex polygon (include/d2d.h
d2d_nlp_solve_free_fence, csrc/nlp_kernels.hip: the NLP_FREE | NLP_KEEP | NLP_FENCE instantiation of nlp_solve_one -- the families' terms of
nlp_merit, nlp_assemble and nlp_apply beside the border, their ratio tests and dual steps in nlp_recover_free) against its CPU statement
tests/nlp_free_fence_ref.py and against the SLSQP arbiter tests/golden/nlp_free_fence_slsqp.npz.

Step by step, on the method of tests/test_gpu_nlp_free.py: after each budget (inner_max, outer_max) of nlp_steps_ref.BUDGETS the step
count must be the statement's exactly, and W, h, u = 1 / h, both families' duals and 2 rho mult must lie within 1e3 x the floor that the
statement shows against itself when every entry of its start moves by an ulp (nlp_steps_ref.measure on nlp_free_fence_ref.ext).  Node
counts 3, 5, 17, 64, 65, 121, 122, 129; per node count the kinds of nlp_free_fence_ref.STEP_CASES in one launch (a disc that binds with
k_dur = 0.5; a corridor edge that binds with k_dur = 0; a disc and a corridor with a y box, k_dur = 2; D2D_MAX_KEEP / D2D_MAX_FENCE rows
with absent ones).  tests/test_nlp_free_fence_cpu.py has the table and how the 'edge' kind came by its narrow corridor.

Measured on the run that added this module (MI355X), per launch over its cases and the eight budgets: the statement's floors, the largest
|(W, h, u, z)_kernel - statement| and the largest error / tolerance (the share of the 1e3 margin the kernel uses):
  3 nodes   (disc, both, many)        floors 2.8e-17 .. 4.1e-12   error 9.1e-12   error / tol 1.0e-02
  5 nodes   (disc, edge, both, many)  floors 1.7e-16 .. 7.2e-12   error 1.3e-11   error / tol 1.0e-02
  17 nodes  (disc, edge, both, many)  floors 3.6e-15 .. 8.1e-12   error 2.5e-12   error / tol 1.3e-02
  64 nodes  (disc, edge, both, many)  floors 1.6e-14 .. 6.8e-12   error 3.0e-12   error / tol 1.2e-03
  65 nodes  (disc, edge, both, many)  floors 2.7e-14 .. 9.6e-12   error 4.3e-12   error / tol 4.7e-03
  121 nodes (disc, edge, both, many)  floors 8.3e-14 .. 9.6e-12   error 3.9e-12   error / tol 2.9e-03
  122 nodes (disc, edge, both, many)  floors 2.1e-14 .. 8.2e-12   error 4.2e-12   error / tol 1.8e-02
  129 nodes (disc, edge, both, many)  floors 4.1e-14 .. 7.2e-12   error 7.5e-12   error / tol 2.1e-02
Every step count, status and multiplier agreed.  Full solves: the 24 problems converge to the statement's cost within 6.9e-10 relative and
to its h within 1.1e-10 (the step counts differ on three of them, 150 / 59 at the most: equal costs by another path).  Pinched box
(h_lo, h_hi within 1e-9 of 0.1, k_dur = 0) against d2d_nlp_solve_fence: the same verdict on all five problems (four CONVERGED, one STALLED),
cost gaps 5.0e-8, 2.5e-9, 5.5e-10, 9.9e-9, 9.6e-9 relative -- the CPU statements show the same five figures.
Power of the comparison, on the committed case table: against a library built with the discs' ratio test skipped in nlp_recover_free
(local build, not committed) the first budget already fails at 5, 64 and 65 nodes:
  'freefence-5-disc (1, 1): floor 1.7e-13, tol 1.7e-10: W off by 8.16e-02 at row 5, plane 1 (the row of h, u)'
  'freefence-64-disc (1, 1): floor 2.7e-14, tol 2.7e-11: W off by 2.84e-02 at row 29, plane 4'
  'freefence-65-disc (1, 1): floor 4.8e-14, tol 4.8e-11: W off by 2.97e-01 at row 26, plane 4'
  'freefence-65-both (1, 1): floor 3.7e-14, tol 3.7e-11: W off by 1.39e-01 at row 63, plane 4'
and every later budget with them (largest error / tol about 1e9); 'freefence-3-disc' and 'freefence-17-both' fail at budget (5, 4).  Only
'disc' and 'both' cases fail, as they must: 'edge' and 'many' hold no disc that binds, so that build computes them as the committed one
does.  At 121, 122 and 129 nodes that build passes (the box and the line search cut those steps before the disc would), and it still
converges on all 24 full solves.
"""
import os

import numpy as np
import pytest

import nlp_fence_ref as E
import nlp_free_fence_ref as FF
import nlp_free_ref as F
import nlp_keepout_ref as K
import nlp_steps_ref as S
from oracle import nlp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nlp_free_fence_slsqp.npz')
COST_RTOL = 1e-7                 # the issue's: |cost - statement's| <= 1e-7 relative at the end of a solve (h likewise, as tests/test_gpu_nlp_free.py)
KEYS = ('cost', 'feas', 'iters', 'status', 'mult', 'h', 'keep_mult', 'fence_mult')


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


def ff_solve(ctx, rows, W0s, fr, discs=None, edges=None, bounds=None, h0=FF.H0, **kw):
    """One d2d_nlp_solve_free_fence launch: rows (B, stride), W0s B x (N, 5), fr (B, 4), discs (B, n, 3) or None, edges (B, n, 4) or None
    -> W (B, N, 5), out (numpy; mult (B, N, 3), h (B,), keep_mult (B, n_keep, N), fence_mult (B, n_edge, N))."""
    W = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    out = ctx.nlp_solve_free_fence(ctx.dev(np.ascontiguousarray(rows)), W, h0, ctx.dev(np.ascontiguousarray(fr)),
                                   discs=None if discs is None else ctx.dev(np.ascontiguousarray(discs)),
                                   edges=None if edges is None else ctx.dev(np.ascontiguousarray(edges)), want_mult=True,
                                   bounds=None if bounds is None else ctx.dev(np.ascontiguousarray(bounds)), **kw)
    ctx.sync()
    return _out(W, out)


def _launch_arrays(got):
    """got: list of (FreeProblem, row, W0, discs, edges) -> rows, W0s, free rows, discs, edges"""
    return (np.stack([g[1] for g in got]), [g[2] for g in got], FF.free_rows([g[0] for g in got]), np.stack([g[3] for g in got]),
            np.stack([g[4] for g in got]))


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
        N = W[b].shape[0]
        We = FF.ext(W[b], dict(h=out['h'][b], u=1.0 / out['h'][b], zk=out['keep_mult'][b], zf=out['fence_mult'][b]))
        dW = np.abs(We - m['W'][0])
        err = float(dW.max())
        worst, ratio = max(worst, err), max(ratio, err / tol)
        if not err <= tol:
            i, c = np.unravel_index(np.argmax(dW), dW.shape)
            bad.append(f'{head}: W off by {err:.2e} at row {i}, plane {c}' + (' (the row of h, u)' if i == N else ' (the duals of discs and edges)' if i > N else ''))
        em = float(np.abs(2 * info['rho'] * out['mult'][b][1:] - info['mult']).max())
        if not em <= tol * 2 * info['rho']:
            bad.append(f'{head}: multipliers off by {em:.2e} > {tol * 2 * info["rho"]:.2e} (rho {info["rho"]:g})')
        cost, feas = case.fn(W[b], out['h'][b])
        if not abs(out['cost'][b] - cost) <= 1e-11 * max(1.0, abs(cost)):
            bad.append(f'{head}: cost {out["cost"][b]!r}, the statement at the same W, h {cost!r}')
        if not abs(out['feas'][b] - feas) <= 1e-12 * max(1.0, 1.0 / out['h'][b]):
            bad.append(f'{head}: feas {out["feas"][b]!r}, the statement at the same W, h {feas!r}')
    return bad, worst, ratio


@pytest.mark.parametrize('N', FF.STEP_N)
def test_kernel_follows_the_statement_step_by_step(ctx, N):
    L = FF.steps_launch(N)
    got = [(g[4], g[1], g[0].W0[0][:N], g[2], g[3]) for g in L.values()]
    cases = [g[0] for g in L.values()]
    rows, W0s, fr, discs, edges = _launch_arrays(got)
    bad, worst, ratio = [], 0.0, 0.0
    for budget in S.BUDGETS:
        W, out = ff_solve(ctx, rows, W0s, fr, discs, edges, inner_max=budget[0], outer_max=budget[1])
        bd, w, r = _compare(cases, budget, W, out)
        bad += bd; worst = max(worst, w); ratio = max(ratio, r)
    fl = [S.measure(c, b)['floor'] for c in cases for b in S.BUDGETS]
    print(f'freefence-{N} ({", ".join(L)}): floors {min(fl):.1e} .. {max(fl):.1e}, largest |(W, h, u, z) - statement| {worst:.2e}, largest error / tol {ratio:.2e}')
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('N', FF.FULL_N)
def test_full_solves_vs_the_statement(ctx, N):
    """Eight full solves per node count in one launch (nlp_free_fence_ref.FULL_CASES): the statement's status and h, its cost within 1e-7
    relative, feas <= 1e-9, h strictly inside its box, every g > 0 at the interior nodes, the duals zero at the end nodes and for absent
    rows, and |z g - mub| <= 1e-12 max(1, z g) on every present constraint (measured: at most 1.9e-14)."""
    got = FF.full_launch(N)
    assert len(got) == 8
    rows, W0s, fr, discs, edges = _launch_arrays(got)
    W, out = ff_solve(ctx, rows, W0s, fr, discs, edges)
    for b, (fp, _, W0, dk, ed) in enumerate(got):
        _, info = FF.solve(fp, W0, FF.H0, dk, ed)
        ia, ja = np.flatnonzero(dk[:, 2] > 0), np.flatnonzero(E.present(ed))
        gd = K.g_values(W[b][1:-1], dk[ia])[0] if len(ia) else np.ones((1, 1))
        ge = E.g_values(W[b][1:-1], ed[ja]) if len(ja) else np.ones((1, 1))
        zk, zf = out['keep_mult'][b], out['fence_mult'][b]
        zg = np.concatenate([(zk[ia][:, 1:-1] * gd).ravel() if len(ia) else np.zeros(0), (zf[ja][:, 1:-1] * ge).ravel() if len(ja) else np.zeros(0)])
        comp = float(np.abs(zg - nlp.MUB_MIN).max())
        print(f'{N}-{b}: status {out["status"][b]} / {info["status"]}, cost {out["cost"][b]:.12f} vs {info["cost"]:.12f}, h {out["h"][b]:.12f} vs {info["h"]:.12f}, '
              f'steps {out["iters"][b]} / {info["inner"]}, feas {out["feas"][b]:.1e}, min g {min(gd.min(), ge.min()):.1e}, largest dual {max(zk.max(), zf.max()):.3g} / '
              f'{max(info["zk"].max(), info["zf"].max()):.3g}, |z g - mub| {comp:.1e}')
        assert out['status'][b] == info['status'] == 1
        assert abs(out['h'][b] - info['h']) <= COST_RTOL * info['h']
        assert abs(out['cost'][b] - info['cost']) <= COST_RTOL * abs(info['cost'])
        assert out['feas'][b] <= 1e-9 and fp.h_lo < out['h'][b] < fp.h_hi
        assert gd.min() > 0.0 and ge.min() > 0.0
        assert not zk[:, [0, -1]].any() and not zf[:, [0, -1]].any()
        assert not np.delete(zk, ia, axis=0).any() and not np.delete(zf, ja, axis=0).any()
        assert max(zk.max(), zf.max()) > 1e-4                                            # a disc or an edge binds ...
        # ... on the central path: the bound that tests/test_nlp_free_fence_cpu.py holds the statement to, |z g - mub| <= 1e-12 max(1, z g) --
        # a thousandth of mub = 1e-9, where the solver's own stopping test would only give 1e-7
        assert comp <= 1e-12 * max(1.0, float(zg.max()))
        assert abs(out['cost'][b] - fp.cost(W[b], 1.0 / out['h'][b])) <= 1e-11 * max(1.0, out['cost'][b])      # discs and edges add nothing to the cost


def test_only_the_free_step_answers(ctx):
    """The two verified cases (17 and 41 nodes, seed 0): d2d_nlp_solve_fence at h = 0.1 on the same rows and tables STALLS,
    d2d_nlp_solve_free_fence CONVERGES."""
    for N, seed in FF.VERIFIED:
        fp, r, W0, discs, edges = FF.detour_problem(N, seed)
        Wd = ctx.dev(np.ascontiguousarray(W0.T[None]))
        fx = ctx.nlp_solve_fence(ctx.dev(r[None]), Wd, FF.H0, ctx.dev(edges[None]), discs=ctx.dev(discs[None]))
        ctx.sync()
        W, out = ff_solve(ctx, r[None], [W0], FF.free_rows([fp]), discs[None], edges[None])
        print(f'{N}/{seed}: fixed status {int(fx["status"][0].item())} feas {float(fx["feas"][0].item()):.2f} after {int(fx["iters"][0].item())} steps; '
              f'free status {out["status"][0]} after {out["iters"][0]} steps, h {out["h"][0]:.5f}')
        assert int(fx['status'][0].item()) == 4 and out['status'][0] == 1
        assert fp.h_lo < out['h'][0] < fp.h_hi and out['feas'][0] <= 1e-9


def test_against_the_slsqp_arbiter(ctx):
    """The kernel against scipy SLSQP over the node values and h itself with the discs and the edges as inequality constraints (5, 9, 17
    nodes): cost and h to tests/test_nlp_free_fence_cpu.py's bounds."""
    from test_nlp_free_fence_cpu import SLSQP_COST_RTOL, SLSQP_H_RTOL
    g = np.load(GOLDEN)
    for k in range(int(g['n_cases'])):
        dk, ed = g[f'c{k}_discs'], g[f'c{k}_edges']
        W, out = ff_solve(ctx, g[f'c{k}_row'][None], [g[f'c{k}_W0']], g[f'c{k}_free_row'][None], dk[None] if len(dk) else None, ed[None] if len(ed) else None)
        dc, dh = abs(out['cost'][0] - g[f'c{k}_cost']) / g[f'c{k}_cost'], abs(out['h'][0] - g[f'c{k}_h']) / g[f'c{k}_h']
        print(f'{g[f"c{k}_name"]}: status {out["status"][0]}, cost off by {dc:.2e} relative, h by {dh:.2e} relative, feas {out["feas"][0]:.1e}')
        assert out['status'][0] == 1 and out['feas'][0] <= 1e-9
        assert dc <= SLSQP_COST_RTOL and dh <= SLSQP_H_RTOL


def test_no_tables_is_the_free_solve_byte_for_byte(ctx):
    """n_keep = n_edge = 0 launches nlp_solve_free_kernel: W, cost, feas, iters, status and h are d2d_nlp_solve_free's bytes."""
    N = 41
    got = [F.leg_problem(N, 300 + s, **kw) for s, kw in ((0, dict(k_dur=0.5)), (1, dict(k_dur=0.5, obstacle=1)), (0, dict(k_dur=2.0)), (1, dict(k_dur=1.0, obstacle=0)))]
    rows, W0s, fr = np.stack([g[1] for g in got]), [g[2] for g in got], F.free_rows([g[0] for g in got])
    W, out = ff_solve(ctx, rows, W0s, fr)
    Wd = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
    ref = ctx.nlp_solve_free(ctx.dev(rows), Wd, FF.H0, ctx.dev(fr), want_mult=True)
    ctx.sync()
    assert (out['status'] == 1).all() and 'keep_mult' not in out and 'fence_mult' not in out
    assert W.tobytes() == Wd.cpu().numpy().transpose(0, 2, 1).tobytes()
    for k in ('cost', 'feas', 'iters', 'status', 'h'):
        assert out[k].tobytes() == ref[k].cpu().numpy().tobytes(), k


def test_a_pinched_box_reproduces_the_fixed_step_verdict(ctx):
    """h_lo and h_hi within 1e-9 relative of h, k_dur = 0: the verdict of d2d_nlp_solve_fence at that h on the same rows and tables.  No
    bit claim: the free kernel reads the equalities at 1 / u and carries the border.  The cost gaps are printed."""
    h = FF.H0
    got = E.full_launch(17) + E.full_launch(41) + [(E.Plain(fp.at(1.0 / h)), r, W0, dk, ed, None) for fp, r, W0, dk, ed in (FF.detour_problem(17, 0),)]
    for N in (17, 41):
        sel = [g for g in got if g[0].pb.N == N]
        rows, W0s = np.stack([g[1] for g in sel]), [g[2] for g in sel]
        discs, edges = np.stack([g[3] for g in sel]), np.stack([g[4] for g in sel])
        fr = np.tile([h * (1 - 5e-10), h * (1 + 5e-10), 0.0, 0.0], (len(sel), 1))
        W, out = ff_solve(ctx, rows, W0s, fr, discs, edges)
        Wd = ctx.dev(np.ascontiguousarray(np.stack([w.T for w in W0s])))
        fx = ctx.nlp_solve_fence(ctx.dev(rows), Wd, h, ctx.dev(edges), discs=ctx.dev(discs))
        ctx.sync()
        st, cf = fx['status'].cpu().numpy(), fx['cost'].cpu().numpy()
        for b in range(len(sel)):
            gap = abs(out['cost'][b] - cf[b]) / abs(cf[b])
            print(f'{N}-{b}: status {out["status"][b]} / fixed {st[b]}, h {out["h"][b]!r}, cost {out["cost"][b]:.12f} vs {cf[b]:.12f}: gap {gap:.2e} relative, '
                  f'steps {out["iters"][b]} / {int(fx["iters"][b].item())}')
            assert out['status'][b] == st[b]
            assert fr[b, 0] < out['h'][b] < fr[b, 1]


def test_refusals_per_problem_in_one_launch(ctx):
    """A bad free row, an end pose inside a disc and an edge with |a| != 1 between good problems: D2D_ST_NONFINITE, NaN cost, feas and h, no
    step, W untouched; the good neighbours solved alike.  The D2D_EINVAL cases of d2d_nlp_solve_fence and of d2d_nlp_solve_free before any
    launch."""
    import ctypes as C
    import d2dhip
    fp, r, W0, dk, ed = FF.full_launch(17)[0]
    good_fr = FF.free_rows([fp])[0]
    bad_fr = good_fr.copy(); bad_fr[0] = -0.05
    inside = dk.copy(); inside[0, :2] = fp.pb.p1[:2]
    long_ = ed.copy(); long_[1, :2] *= 1.0 + 1e-9
    frs = [good_fr, bad_fr, good_fr, good_fr, good_fr, good_fr, good_fr]
    dks = [dk, dk, dk, inside, dk, dk, dk]
    eds = [ed, ed, ed, ed, ed, long_, ed]
    B = len(frs)
    W, out = ff_solve(ctx, np.stack([r] * B), [W0] * B, np.stack(frs), np.stack(dks), np.stack(eds))
    print(f'status {out["status"].tolist()}')
    for b in range(B):
        if b in (1, 3, 5):
            assert out['status'][b] == d2dhip.ST_NONFINITE and np.isnan(out['cost'][b]) and np.isnan(out['feas'][b]) and np.isnan(out['h'][b]) and out['iters'][b] == 0, b
            assert np.array_equal(W[b], W0), b
        else:
            assert out['status'][b] == 1 and np.array_equal(W[b], W[0]) and out['cost'][b] == out['cost'][0] and out['h'][b] == out['h'][0], b
    assert FF.solve(fp, W0, FF.H0, inside, ed)[1]['status'] == FF.solve(fp, W0, FF.H0, dk, long_)[1]['status'] == d2dhip.ST_NONFINITE
    with pytest.raises(d2dhip.D2DError, match=rf'error -1: .*n_edge = {d2dhip.MAX_FENCE + 1} outside'):
        ff_solve(ctx, r[None], [W0], good_fr[None], dk[None], np.zeros((1, d2dhip.MAX_FENCE + 1, 4)))
    with pytest.raises(d2dhip.D2DError, match=rf'error -1: .*n_keep = {d2dhip.MAX_KEEP + 1} outside'):
        ff_solve(ctx, r[None], [W0], good_fr[None], np.zeros((1, d2dhip.MAX_KEEP + 1, 3)), ed[None])
    with pytest.raises(d2dhip.D2DError, match='error -1: .*serial = 1'):
        Wd = ctx.dev(np.ascontiguousarray(W0.T[None]))
        ctx._nlp_core(ctx.lib.d2d_nlp_solve_free_fence, ctx.dev(r[None]), Wd, FF.H0, (10.0, 0.1, 1e-9, 1e-9, 1e-7, d2dhip.NLP_INNER_MAX, d2dhip.NLP_OUTER_MAX, 1), None,
                      free_rows=ctx.dev(good_fr[None]), keep=ctx.dev(dk[None]), fence=ctx.dev(ed[None]))
    lib, N = ctx.lib, fp.pb.N
    Wd = ctx.dev(np.ascontiguousarray(W0.T[None])); work = ctx.empty(lib.d2d_nlp_free_workspace_doubles(N)); cost = ctx.empty(1); feas = ctx.empty(1); hout = ctx.empty(1)
    frd = ctx.dev(good_fr[None])
    args = [ctx.h, 1, N, FF.H0, ctx.dev(r[None]).data_ptr(), None, frd.data_ptr(), Wd.data_ptr(), work.data_ptr(), None, cost.data_ptr(), feas.data_ptr(), None, None,
            hout.data_ptr()]
    keep0, fence0 = d2dhip.KeepOutC(0, 0, None), d2dhip.FenceC(0, 0, None)
    assert lib.d2d_nlp_solve_free_fence(*args, C.byref(keep0), None, None, None) == -1                                              # fence NULL
    assert lib.d2d_nlp_solve_free_fence(*args, None, None, C.byref(fence0), None) == -1                                             # keep NULL
    assert lib.d2d_nlp_solve_free_fence(*args, C.byref(keep0), None, C.byref(d2dhip.FenceC(4, 0, None)), work.data_ptr()) == -1     # edges NULL with n_edge > 0
    assert lib.d2d_nlp_solve_free_fence(*args, C.byref(keep0), None, C.byref(d2dhip.FenceC(4, 0, work.data_ptr())), None) == -1     # fwork NULL with n_edge > 0
    assert lib.d2d_nlp_solve_free_fence(*args, C.byref(d2dhip.KeepOutC(2, 0, work.data_ptr())), None, C.byref(fence0), None) == -1  # kwork NULL with n_keep > 0
    assert lib.d2d_nlp_solve_free_fence(*args, C.byref(d2dhip.KeepOutC(-1, 0, None)), None, C.byref(fence0), None) == -1
    ctx.sync()
    assert np.array_equal(Wd.cpu().numpy()[0].T, W0)


def test_order_only_schedules(ctx):
    """The eight 41-node problems four times over, B = 32: a reversed hand-out order gives bit-identical W, h, duals, cost, iters and status."""
    import torch
    got = FF.full_launch(41) * 4
    rows, W0s, fr, discs, edges = _launch_arrays(got)
    B = len(got)
    W1, o1 = ff_solve(ctx, rows, W0s, fr, discs, edges)
    order = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=ctx.device).contiguous()
    W2, o2 = ff_solve(ctx, rows, W0s, fr, discs, edges, order=order)
    assert (o1['status'] == 1).all()
    assert np.array_equal(W1, W2) and np.array_equal(W1[:8], W1[8:16])
    for k in KEYS:
        assert np.array_equal(o1[k], o2[k]), k


def test_planner_on_exp14_with_a_disc_a_fence_and_a_window(ctx):
    """single_opt_planner.Planner on exp_14 with a KeepOut across the leg, a GeoFence round it and t1_window = (10, 24) s: CONVERGED, the
    duration inside the window, both clearances at least their margins (the disc lowered with h_hi).  The same scenario with t1 fixed at
    t1_lo = 10 s cannot converge: the leg is 159 m and v_max 15 m/s.  Without disc and fence t1_window returns t1_free's plan bit for bit."""
    import d2d.optyplan_scenarios as sc
    import single_opt_planner as sop
    from test_nlp_fence_cpu import scenario_fence
    from test_nlp_keepout_cpu import _disc_across, _exp14
    e = sc.exp_14
    ko = _disc_across(e)
    gf = scenario_fence(e, 60.0, 60.0, 1.0)
    win = (10.0, 24.0)
    p = sop.Planner(_exp14(keep_out=[ko], fence=gf, t1_window=win), backend='auto')
    p.run()
    print(f'exp_14 window {win} round {ko} inside {gf}: status {p.info["status"]}, duration {p.duration!r}, time_step {p.time_step!r}, cost {p.info["obj_val"]!r}, '
          f'clearances {p.info["keep_out_clearance"]} / {min(p.info["fence_clearance"]):.4f}, steps {p.info["iters"]}')
    assert p.info['status'] == 1 and p.info['backend_used'] == 'nlp' and p.info['feas'] <= 1e-9
    assert win[0] < p.duration < win[1] and p.info['duration'] == p.duration and p.info['time_step'] == p.time_step and p.sol_time[-1] == p.duration
    assert p.info['keep_out_clearance'][0] >= ko.margin and min(p.info['fence_clearance']) >= gf.margin
    assert e.v_constraint[0] <= p.sol_v.min() and p.sol_v.max() <= e.v_constraint[1]
    q = sop.Planner(_exp14(keep_out=[ko], fence=gf, t1=win[0]), backend='nlp')
    q.run()
    print(f'the same with t1 = {win[0]} fixed: status {q.info["status"]}, feas {q.info["feas"]:.2e}')
    assert q.info['status'] != 1
    a, b = sop.Planner(_exp14(t1_window=win), backend='nlp'), sop.Planner(_exp14(t1_free=win), backend='nlp')
    a.run(); b.run()
    assert a.info['status'] == 1 and np.array_equal(a.solution, b.solution) and a.duration == b.duration


def test_plan_batch_window_matches_a_direct_solve(ctx):
    """plan_batch(window=, keep_out=, fence=) for four problems returns the direct solve on the same rows and tables, h and free_rows as
    free_time's; a list of KeepOut is lowered with h_hi."""
    import d2d.opty_utils as ou
    import d2dhip
    import full_sim
    N = 41
    got = FF.full_launch(N)[:4]
    rows, W0s, fr, discs, edges = _launch_arrays(got)
    W0 = np.ascontiguousarray(np.stack([w.T for w in W0s]))
    out = full_sim.plan_batch(rows, N, (N - 1) * FF.H0, 1.0 / N, backend='nlp', W0=W0, h=FF.H0, window=fr[:, :2], kdur=fr[:, 2], keep_out=discs, fence=edges)
    W, ref = ff_solve(ctx, rows, W0s, fr, discs, edges)
    ctx.sync()
    assert out['entry'] == 'nlp_solve_free_fence' and np.array_equal(out['free_rows'], fr) and (ref['status'] == 1).all()
    assert np.array_equal(out['h'].cpu().numpy(), ref['h']) and np.array_equal(out['cost'].cpu().numpy(), ref['cost'])
    assert np.array_equal(out['W'].cpu().numpy().transpose(0, 2, 1), W)
    assert np.array_equal(out['keep_mult'].cpu().numpy(), ref['keep_mult']) and np.array_equal(out['fence_mult'].cpu().numpy(), ref['fence_mult'])
    ko = ou.KeepOut(discs[0, 0, :2], 0.5 * discs[0, 0, 2], margin=0.1)
    o2 = full_sim.plan_batch(rows[:1], N, (N - 1) * FF.H0, 1.0 / N, backend='nlp', W0=W0[:1], h=FF.H0, window=(0.05, 0.2), keep_out=[ko])
    assert o2['keep'][0, 0, 2] == K.lowered_radius(ko.r, ko.margin, rows[0, d2dhip.SC_VMAX], 0.2) and o2['fence_mult'] is None
