"""d2d_nlp_guess_dubins (csrc/nlp_guess.hip) on the GPU against its CPU statement tests/nlp_guess_ref.py on the committed parity
cases (tests/nlp_guess_cases.py, every one of them determined: tests/test_nlp_guess_cpu.py), its refusals and guards, the bytes it
must not depend on, and the point of it: fewer Newton steps of d2d_nlp_solve to the same minima.

Tolerance of the parity test: measured, per case and quantity -- the statement's own floor (nlp_guess_ref.floors: the largest change
of the quantity when an end-pose entry moves by one ulp or the result of one transcendental moves by one ulp) times the project's
margin of 1e3.  A quantity whose floor is 0 is one the rule reproduces exactly (the speed of a FIT is a point of the search grid, the
speed of a SHORT is v_hi) and must be equal."""
import ctypes as C

import numpy as np
import pytest

import nlp_guess_cases as GC
import nlp_guess_ref as GR

pytestmark = pytest.mark.gpu
MARGIN = 1e3
GUARD = 512          # doubles: 4 KiB
_FLOORS = {}


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    return d2dhip.default_context()


def _dev(ctx, a):
    return None if a is None else ctx.dev(np.ascontiguousarray(a))


def _launch(ctx, rows, N, h, bounds=None, v_pref=None, **kw):
    W, out = ctx.nlp_guess_dubins(_dev(ctx, rows), N, h, bounds=_dev(ctx, bounds), v_pref=_dev(ctx, v_pref), **kw)
    ctx.sync()
    return W.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


def _floor(ci, variant, N):
    key = (ci, variant, N)
    if key not in _FLOORS:
        c = GC.CASES[ci]
        opts = variant == 'opts'
        _FLOORS[key] = GR.floors(GC.row(c), N, GC.step(N), c[5] if opts else None, c[6] if opts else None)
    return _FLOORS[key]


@pytest.mark.parametrize('variant', GC.VARIANTS)
@pytest.mark.parametrize('N', GC.NS)
def test_parity_with_the_statement(ctx, N, variant):
    """B in {1, 63, 65}: the wave tail; N: two nodes, the one-node interior, the strided fill at and past a wavefront.  Status and
    word equal; every quantity within 1e3 floors of the statement."""
    h = GC.step(N)
    worst, fl_lo, fl_hi, err_hi = 0.0, np.inf, 0.0, 0.0
    for B in GC.BS:
        rows, bounds, v_pref, want = GC.batch(B, variant)
        Wr, ref = GR.guess(rows, N, h, bounds, v_pref)
        W, got = _launch(ctx, rows, N, h, bounds, v_pref)
        assert np.array_equal(got['status'], ref['status']) and np.array_equal(got['word'], ref['word']), (B, got['status'], ref['status'])
        assert np.array_equal(np.stack([got['status'], got['word']], 1), want)
        for b in range(B):
            ci = b % len(GC.CASES)
            fl = _floor(ci, variant, N)
            err = GR.difference(W[b], {k: got[k][b] for k in ('v', 'rho', 'L', 't_nat')}, Wr[b], {k: ref[k][b] for k in ('v', 'rho', 'L', 't_nat')})
            bad = err > MARGIN * fl
            assert not bad.any(), (B, b, ci, [(q, f, e) for q, f, e, x in zip(GR.QUANTITIES, fl, err, bad) if x])
            pos = fl > 0.0
            worst = max(worst, float((err[pos] / (MARGIN * fl[pos])).max(initial=0.0)))
            fl_lo, fl_hi, err_hi = min(fl_lo, fl[pos].min()), max(fl_hi, fl.max()), max(err_hi, err.max())
    print('guess parity N=%d %s: floors %.1e ... %.1e, largest error %.1e, largest error / tolerance %.1e' % (N, variant, fl_lo, fl_hi, err_hi, worst))


def _guarded(ctx, n, torch_dtype, fill):
    import torch
    per = 8 // torch.empty(0, dtype=torch_dtype).element_size()
    full = torch.full(((2 * GUARD) * per + n,), fill, dtype=torch_dtype, device=ctx.device)
    return full, full[GUARD * per:GUARD * per + n]


def _raw_call(ctx, B, N, h, scen, W, out_ptrs, bounds=None, v_pref=None, kappa=0.9, waves=0, opts=True, out=True):
    import d2dhip
    o = d2dhip.NlpGuessOut(*[None if p is None else p.data_ptr() for p in out_ptrs])
    op = d2dhip.NlpGuessOpts(kappa, None if bounds is None else bounds.data_ptr(), None if v_pref is None else v_pref.data_ptr(), waves, 0)
    return ctx.lib.d2d_nlp_guess_dubins(ctx.h, B, N, h, None if scen is None else C.c_void_p(scen.data_ptr()), C.byref(op) if opts else None,
                                        None if W is None else C.c_void_p(W.data_ptr()), C.byref(o) if out else None)


def test_optional_outputs_and_guards(ctx):
    """Every optional output NULL, the out struct NULL, opts NULL, and all outputs: the same W bytes; nothing is written outside W
    and the outputs (4 KiB guards); refused rows keep their W bytes."""
    import torch
    N, h = 65, GC.step(65)
    good, _, _, _ = GC.batch(9, 'plain')
    rows = np.concatenate([good[:5], GC.refused_rows(), good[5:]])
    refused = np.arange(5, 5 + len(GC.REFUSALS))
    B = rows.shape[0]
    scen = ctx.dev(rows)
    results = []
    for mode in ('all', 'none', 'no-struct', 'no-opts'):
        Wf, W = _guarded(ctx, B * 5 * N, torch.float64, -7.25)
        outs = [_guarded(ctx, B, torch.int32 if k in ('status', 'word') else torch.float64, -3) for k in ('status', 'word', 'v', 'rho', 'L', 't_nat')]
        ptrs = [o[1] if mode == 'all' else None for o in outs]
        assert _raw_call(ctx, B, N, h, scen, W, ptrs, opts=mode != 'no-opts', out=mode != 'no-struct') == 0
        ctx.sync()
        Wh = Wf.cpu().numpy()
        assert np.all(Wh[:GUARD] == -7.25) and np.all(Wh[-GUARD:] == -7.25), mode
        body = Wh[GUARD:-GUARD].reshape(B, 5, N)
        assert np.all(body[refused] == -7.25), mode
        assert not np.any(body[np.setdiff1d(np.arange(B), refused)][:, :3] == -7.25), mode
        for (full, view), k in zip(outs, ('status', 'word', 'v', 'rho', 'L', 't_nat')):
            fh, per = full.cpu().numpy(), 2 if full.dtype == torch.int32 else 1
            assert np.all(fh[:GUARD * per] == -3) and np.all(fh[-GUARD * per:] == -3), (mode, k)
            assert mode == 'all' or np.all(fh == -3), (mode, k)
        results.append((body.tobytes(), [o[1].cpu().numpy() for o in outs]))
    assert all(r[0] == results[0][0] for r in results)
    st, word, v = results[0][1][0], results[0][1][1], results[0][1][2]
    assert np.all(st[refused] == GR.INVALID) and np.all(word[refused] == -1) and np.all(np.isnan(v[refused]))
    Wr, ref = GR.guess(rows, N, h)
    assert np.array_equal(st, ref['status']) and np.array_equal(word, ref['word'])


def test_einval_leaves_everything_untouched(ctx):
    import d2dhip
    import torch
    N, h = 17, GC.step(17)
    rows, _, _, _ = GC.batch(3, 'plain')
    scen = ctx.dev(rows)
    W = ctx.dev(np.full((3, 5, N), -7.25))
    outs = [torch.full((3,), -3, dtype=torch.int32 if k in ('status', 'word') else torch.float64, device=ctx.device) for k in d2dhip.GUESS_OUT]
    bad = (dict(B=0), dict(N=1), dict(h=0.0), dict(h=-0.1), dict(h=float('nan')), dict(h=float('inf')), dict(kappa=0.0), dict(kappa=1.5),
           dict(kappa=float('nan')), dict(waves=-1), dict(scen=None), dict(W=None))
    for kw in bad:
        a = dict(B=3, N=N, h=h, scen=scen, W=W)
        a.update({k: v for k, v in kw.items() if k in a})
        rc = _raw_call(ctx, a['B'], a['N'], a['h'], a['scen'], a['W'], outs, kappa=kw.get('kappa', 0.9), waves=kw.get('waves', 0))
        assert rc == -1, (kw, rc)                   # D2D_EINVAL
        assert b'd2d_nlp_guess_dubins' in ctx.lib.d2d_last_error()
    ctx.sync()
    assert np.all(W.cpu().numpy() == -7.25) and all(np.all(o.cpu().numpy() == -3) for o in outs)
    with pytest.raises(d2dhip.D2DError):
        ctx.nlp_guess_dubins(scen, N, h, kappa=2.0)


def test_same_bytes_from_call_to_call_and_for_two_grids(ctx):
    N, h = 129, GC.step(129)
    rows, bounds, v_pref, _ = GC.batch(65, 'opts')
    runs = [_launch(ctx, rows, N, h, bounds, v_pref, waves=w) for w in (0, 0, 8, 1)]
    for W, out in runs[1:]:
        assert W.tobytes() == runs[0][0].tobytes() and all(out[k].tobytes() == runs[0][1][k].tobytes() for k in out)


def test_fewer_newton_steps_to_the_same_minima(ctx):
    """64 problems of synth.nlp_problems(seed=0), 121 nodes, through Context.nlp_solve from the host dog-leg and from the device
    Dubins start: the same statuses, the converged costs within 1e-7, at most 0.75 of the Newton steps, a shorter longest problem."""
    from d2dhip import synth
    B, N = 64, 121
    rows, W0, h = synth.nlp_problems(B, N, seed=0)
    scen = ctx.dev(rows)
    Wt = ctx.dev(W0)
    tri = ctx.nlp_solve(scen, Wt, h)
    Wd, g = ctx.nlp_guess_dubins(scen, N, h)
    dub = ctx.nlp_solve(scen, Wd, h)
    ctx.sync()
    st_t, st_d = tri['status'].cpu().numpy(), dub['status'].cpu().numpy()
    it_t, it_d = tri['iters'].cpu().numpy(), dub['iters'].cpu().numpy()
    ct, cd = tri['cost'].cpu().numpy(), dub['cost'].cpu().numpy()
    print('guess steps: dog-leg %d, Dubins %d (%.3f); longest %d -> %d; statuses %s; guess %s' % (
        it_t.sum(), it_d.sum(), it_d.sum() / it_t.sum(), it_t.max(), it_d.max(), np.bincount(st_t, minlength=5), np.bincount(g['status'].cpu().numpy(), minlength=6)))
    assert np.array_equal(st_t, st_d), (st_t, st_d)
    conv = st_t == 1
    assert conv.sum() >= 48 and np.abs(ct[conv] - cd[conv]).max() <= 1e-7, np.abs(ct[conv] - cd[conv]).max()
    assert it_d.sum() <= 0.75 * it_t.sum(), (it_t.sum(), it_d.sum())
    assert it_d.max() < it_t.max()


def test_planner_from_the_dubins_guess_reaches_the_reference_cost():
    """single_opt_planner.Planner(exp_14, backend='nlp') from get_initial_guess('dubins'): the committed IPOPT cost, to the tolerance
    tests/test_gpu_nlp.py uses for the dog-leg; the multi planner gives each aircraft its own path."""
    import d2d.optyplan_scenarios as d2oscen
    import single_opt_planner as sop
    p = sop.Planner(d2oscen.exp_14, initialize=True, backend='nlp')
    p.configure(1e-5, 1500)
    g = p.get_initial_guess('dubins')
    assert g.shape == (605,) and list(p.guess_status) in ([GR.FIT], [GR.SHORT])
    assert (g[0], g[121], g[242]) == tuple(d2oscen.exp_14.p0[:3]) and (g[120], g[241], g[362]) == tuple(d2oscen.exp_14.p1[:3])
    p.run(g)
    c = d2oscen.exp_14.cost.cost(p.solution, p)
    assert p.info['status'] == 1 and abs(c - 5.02972817) <= 1e-6 * 5.02972817, (p.info, c)
    with pytest.raises(NotImplementedError, match='dubins'):
        sop.Planner(d2oscen.exp_14, initialize=True, backend='fit').get_initial_guess('dubins')
    import multi_opt_planner as mop
    scen = mop.trap_4
    keep = scen.t1, scen.p0s, scen.p1s
    try:
        scen.t1 = 6
        scen.p0s = ((0, 40, 0, 0, 12), (25, 40, 0, 0, 12), (25, -40, 0, 0, 12), (0, -40, 0, 0, 12))
        scen.p1s = ((75, 40, 0, 0, 12), (100, 40, 0.3, 0, 12), (100, -40, -0.3, 0, 12), (75, -40, 0, 0, 12))
        m = mop.Planner(scen, initialize=True, backend='nlp')
        gm = m.get_initial_guess('dubins')
        assert gm.shape == (5 * 4 * 61,) and len(m.guess_status) == 4
        for i in range(4):
            assert (gm[m._slice_x[i]][0], gm[m._slice_y[i]][0], gm[m._slice_psi[i]][-1]) == (scen.p0s[i][0], scen.p0s[i][1], scen.p1s[i][2])
            assert gm[m._slice_v[i]].min() >= scen.v_constraint[0] and gm[m._slice_v[i]].max() <= scen.v_constraint[1]
    finally:
        scen.t1, scen.p0s, scen.p1s = keep


@pytest.mark.parametrize('n_ac', (1, 2))
def test_plan_batch_from_the_device_guess_equals_the_array(ctx, n_ac):
    """plan_batch(W0='dubins') guesses the rows on the device, each aircraft row on its own, and returns bit for bit the plan of
    plan_batch(W0=<the same guess as an array>); with via= it is refused by name."""
    import full_sim
    from d2dhip import synth
    N = 61
    if n_ac == 1:
        rows, _, h = synth.nlp_problems(6, N, seed=3)
    else:
        rows, h = synth.circle_group_scenarios(2, 3, 12.0, K=N, seed=1).reshape(6, -1), 12.0 / (N - 1)
    a = full_sim.plan_batch(rows, N, (N - 1) * h, None, backend='nlp', W0='dubins', h=h, n_ac=n_ac)
    Wg, g = ctx.nlp_guess_dubins(ctx.dev(rows), N, h)
    ctx.sync()
    b = full_sim.plan_batch(rows, N, (N - 1) * h, None, backend='nlp', W0=Wg.cpu().numpy(), h=h, n_ac=n_ac)
    ctx.sync()
    assert np.array_equal(a['guess_status'].cpu().numpy(), g['status'].cpu().numpy()) and 'guess_status' not in b
    for k in ('W', 'cost', 'feas', 'iters', 'status'):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert a['entry'] == b['entry']
    with pytest.raises(NotImplementedError, match='via'):
        full_sim.plan_batch(rows, N, (N - 1) * h, None, backend='nlp', W0='dubins', h=h, n_ac=n_ac, via=[[] for _ in range(6)])
    with pytest.raises(NotImplementedError, match='nlp'):
        full_sim.plan_batch(rows, N, (N - 1) * h, 0.1 / N, backend='fit', W0='dubins')
