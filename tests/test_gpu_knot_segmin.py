"""GPU: the knot kernel's instantiation with a compile-time floor on the segment length (csrc/fit_knot.hip: SEGMIN, J^T r inside
the MFMA pass) against its generic instantiation, bit for bit.  D2D_FIT_ABLATE & 64 (a diagnostic switch, read at every launch)
forces the generic one; cost, q, trial counts, status and the evaluation count of 64 fits must be np.array_equal.

K (tests/test_knot_segmin_cpu.py states the geometry): 23, the smallest the plan accepts (segments of 3 and 4: generic either
way); 48, equal segments of 8, the first K with the floor (no sample past it); 54 | 55, either side of the SEG9 boundary (longest
segment 9 | 10: one | three predicated k-steps past the floor); 50, the bench's, also with so_lambda = 0 and in CostBank's max mode
(second-order evaluations, the kept phi row).  No K <= 64 has segments that differ by two samples."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ITER = 150
FIELDS = ('cost', 'q', 'iters', 'status', 'evals')


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    c = d2dhip.Context(0)
    yield c
    c.close()


def _scenarios(name):
    import bench
    from d2dhip import synth
    if name in ('k50', 'so0', 'bankmax'):
        dur, wref = bench._plan_consts()
        sc = synth.variant_scenarios('bankmax', 64, K=bench.K) if name == 'bankmax' else bench.bench_scenarios(4096)[:64]
        return bench.K, dur, wref, sc
    K = int(name[1:])
    dur = synth.planner_timing(0, (K - 1) / 10.0, 10)[2]
    return K, dur, synth.default_wref(0.1, K), synth.synth_scenarios(64, seed=5, obj_scale=0.1, K=K, dist_range=(30. * dur / 4.9, 55. * dur / 4.9))


def _solve(ctx, name):
    import d2dhip
    K, dur, wref, sc = _scenarios(name)
    dsc = ctx.dev(sc)
    plan = d2dhip.FitPlan(ctx, 6, K, dur, wref, kernel='knot')
    try:
        assert plan.kernel == 'knot'
        q = plan.init(dsc)
        kw = {'so_lambda': 0.0} if name == 'so0' else {}
        cost, iters, status, stats = plan.solve(dsc, q, max_iter=MAX_ITER, **kw)
        return {'cost': cost.cpu().numpy(), 'q': q.cpu().numpy(), 'iters': iters.cpu().numpy(), 'status': status.cpu().numpy(),
                'evals': np.asarray(stats, dtype=np.float64)[3:4].copy()}
    finally:
        plan.close()


@pytest.mark.parametrize('name', ['k23', 'k48', 'k54', 'k55', 'k50', 'so0', 'bankmax'])
def test_floor_and_generic_instantiations_agree_bit_for_bit(ctx, monkeypatch, name):
    import d2dhip
    K, dur, _, _ = _scenarios(name)
    floor = d2dhip.knot_segments(6, K, dur)[3]
    assert floor == (8 if K >= 48 else 0)
    monkeypatch.delenv('D2D_FIT_ABLATE', raising=False)
    spec = _solve(ctx, name)
    monkeypatch.setenv('D2D_FIT_ABLATE', '64')
    gen = _solve(ctx, name)
    assert spec['iters'].max() <= MAX_ITER and spec['iters'].min() >= 1 and int(spec['evals'][0]) >= 2 * 64
    for k in FIELDS:
        a, b = spec[k], gen[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
            pytest.fail(f'{name}.{k}: {len(bad)} of {len(a)} rows differ between the two instantiations (first: {bad[:8].tolist()})')
