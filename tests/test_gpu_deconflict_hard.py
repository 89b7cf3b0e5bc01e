"""GPU: full_sim.deconflict_plans(hard=True) and plan_batch(deconflict=dict(..., hard=True)) on the two shared worlds of
tests/test_gpu_deconflict.py, MARGIN 0, against the loop's CPU statement (nlp_keepout_moving_ref.deconflict_hard).

The discs are hard constraints of the re-solve with node radius sqrt(d_sep^2 + step_max^2) + chord_err, so near_dist >= d_sep is not a
tuned number here but the theorem of deconflict_plans' docstring: it is asserted with margin 0, where the soft loop on the same
scenarios ends at 2.86 m (tests/test_nlp_keepout_moving_cpu.py).  Tolerances against the CPU statement: status equal, cost within 1e-7
relative (of max(cost, 1e-3)), nodes within 1e-4."""
import numpy as np
import pytest

import nlp_keepout_moving_ref as KM
import nlp_moving_ref as M
from oracle import nlp
from test_gpu_deconflict import scenario, N, H, D_SEP, D_LOOK, STEP_MAX

pytestmark = pytest.mark.gpu
DEC = dict(d_sep=D_SEP, margin=0.0, d_look=D_LOOK, step_max=STEP_MAX)


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    return d2dhip.default_context()


@pytest.fixture(scope='module', params=[1, 2])
def case(request, ctx):
    import full_sim
    rows, n_ac = scenario(request.param)
    W0 = np.stack([M.straight_guess(r, N).T for r in rows])
    plan = lambda **kw: full_sim.plan_batch(rows, N, (N - 1) * H, 1.0, backend='nlp', W0=W0, h=H, n_ac=n_ac, **kw)      # noqa: E731
    indep = plan()
    ctx.sync()
    Wi = indep['W'].cpu().numpy()
    out = plan(deconflict=dict(DEC, hard=True))
    ctx.sync()
    Wc = [nlp.solve(nlp.problem_from_row(r, N, H), M.straight_guess(r, N))[0] for r in rows]
    Wr, ref = KM.deconflict_hard(rows, Wc, n_ac, H, D_SEP, 0.0, D_LOOK, STEP_MAX)
    return dict(k=request.param, rows=rows, n_ac=n_ac, R=len(rows) // n_ac, indep=indep, Wi=Wi, out=out, W=out['W'].cpu().numpy(),
                info=out['deconflict'], Wr=Wr, ref=ref)


def test_the_theorem_holds_with_margin_zero(ctx, case):
    n_ac, R, W, Wi, info = case['n_ac'], case['R'], case['W'], case['Wi'], case['info']
    assert W[:n_ac].tobytes() == Wi[:n_ac].tobytes()                       # the top formation keeps its plan, byte for byte
    a = ctx.fleet_audit(case['out']['W'], n_ac, H, D_LOOK, STEP_MAX, d_safe=D_SEP, layout='plan')
    ctx.sync()
    near = a['near_dist'].cpu().numpy()
    print('after', near, 'rounds', info['rounds'], info['replanned'])
    assert not info['truncated'] and info['not_converged'] == [] and info['refused'] == [] and info['unresolved'] == []
    assert info['rounds'] < 4                                               # a fixed point, not the round limit
    assert (near >= D_SEP).all()
    for f in range(1, R):
        assert np.abs(W[f * n_ac:(f + 1) * n_ac] - Wi[f * n_ac:(f + 1) * n_ac]).max() > 1.0, f


def test_the_loop_is_the_cpu_statements(ctx, case):
    info, ref = case['info'], case['ref']
    assert [s['forms'].cpu().numpy().tolist() for s in info['solves']] == ref['replanned'] == ([[1]] if case['k'] == 1 else [[1, 2], [2]])
    assert ref['refused'] == [] and ref['not_converged'] == []
    for s, costs, status in zip(info['solves'], ref['costs'], ref['status']):
        got, want = s['cost'].cpu().numpy(), np.concatenate(costs)
        rel = np.abs(got - want) / np.maximum(want, 1e-3)
        print('costs', got, want, 'rel', rel.max(), 'feas', s['feas'].cpu().numpy().max())
        assert (s['status'].cpu().numpy() == np.concatenate(status)).all() and (np.concatenate(status) == 1).all()
        assert rel.max() <= 1e-7 and s['feas'].cpu().numpy().max() <= 1e-8
    dn = max(np.abs(case['W'][b].T - case['Wr'][b]).max() for b in range(len(case['Wr'])))
    print('nodes', dn)
    assert dn <= 1e-4
    import fleet_audit_ref as FL
    assert (FL.audit(np.stack(case['Wr'], axis=2), case['n_ac'], H, D_LOOK, STEP_MAX)['near_dist'] >= D_SEP).all()


def test_the_direct_call_and_hard_false(ctx, case):
    """deconflict_plans called directly gives plan_batch's bytes; hard=False gives the bytes of the call without the keyword."""
    import full_sim
    rows, n_ac = case['rows'], case['n_ac']
    dsc = ctx.dev(rows)                                                     # (the rows carry no collision term: no masks to write)
    W = ctx.dev(case['Wi'].copy())
    _, info = full_sim.deconflict_plans(ctx, dsc, W, H, n_ac, hard=True, **DEC)
    ctx.sync()
    assert W.cpu().numpy().tobytes() == case['W'].tobytes() and info['replanned'] == case['info']['replanned']
    Wa, Wb = ctx.dev(case['Wi'].copy()), ctx.dev(case['Wi'].copy())
    _, ia = full_sim.deconflict_plans(ctx, dsc, Wa, H, n_ac, **DEC)
    _, ib = full_sim.deconflict_plans(ctx, dsc, Wb, H, n_ac, hard=False, **DEC)
    ctx.sync()
    assert Wa.cpu().numpy().tobytes() == Wb.cpu().numpy().tobytes() and ia['replanned'] == ib['replanned'] and ib['refused'] == []
    assert ia['audit']['near_dist'].cpu().numpy().tobytes() == ib['audit']['near_dist'].cpu().numpy().tobytes()
    assert np.nanmin(ia['audit']['near_dist'].cpu().numpy()) < D_SEP       # the soft loop at margin 0 ends below the bar
