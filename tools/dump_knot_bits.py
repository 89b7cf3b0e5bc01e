"""The knot kernel's results on a fixed set of small fit families, bit for bit: tests/golden/knot_parent_bits.npz.

    python tools/dump_knot_bits.py [OUT.npz]          (D2D_LIB=<library> selects the build, as for every A/B run)

The fixture was written ONCE, with the build of the commit BEFORE the round-7 pass over the solver loop, and is what
tests/test_gpu_knot_bits.py compares every later build with: a change of csrc/fit_knot.hip or of damped_solve that is meant to remove
work only must leave every array below np.array_equal.  A change that is MEANT to alter a rounding re-writes the fixture with this
tool and says so.

Families (max_iter = 150 everywhere; name -> what it reaches):
  bench     192 bench scenarios, K = 50          the SEG9 instantiation: Gauss-Newton steps inside and outside the region, lmpar, the finish
  k40, k64  64 each of the other-K scenarios     K = 64 is the generic (non-SEG9) instantiation
  so0       64 bench scenarios, so_lambda = 0    the option's Gauss-Newton setting (the MINPACK path's finish is second-order whatever it says)
  bankmax   64 CostBank-max scenarios            the piecewise-smooth cost: rejected trials, long finishes
  resume    64 bench scenarios, 7 trials a launch every fit goes through the resume path (lm[] state, the kept knot vector)
Per family: cost, q (float64), iters, status (int32) and stats (float64[3]: max |J^T r| over the family, fits not converged, evaluations
-- d2d_fit_solve's stats[1 .. 3]; stats[0], the cost sum, is accumulated with atomics in an order that is not fixed, and `cost` holds
its terms).  The per-fit count of factorisations, lm[7], stays inside the plan -- no entry point of the library returns it -- so the
evaluation count and the trial counts of `iters` are what pins the path a fit took.

    python tools/dump_knot_bits.py --r9 [OUT.npz]     tests/golden/knot_r9_parent_bits.npz (tests/test_gpu_knot_metric_row.py)

A second, smaller fixture, written ONCE with the build of the commit before round 9 (the metric's zero row, the packed
column scaling of the back substitution).  32 fits a case, max_iter = 40: at that size every fit starts at once, so the hand-out
order plays no part, and within the first trial of every fit both kinds of solve occur, Gauss-Newton (no damping on any lane) and
damped.  The scenario families are those of tests/test_gpu_knot_segmin.py:
  k23, k48, k50, k55, k64   the generic instantiation, every segment at the floor, the bench's K, the first K past SEG9, the longest
  so0, bankmax              K = 50 with so_lambda = 0, and in CostBank's max mode
and the three other kernels that share damped_solve (they pin its back substitution outside the knot kernel):
  fused    K = 50 with d2d_fit_plan_opts.kernel = FUSED (fit_lm_kernel)
  long     K = 121 (fit_lm_long_kernel)
  groups   2 aircraft x 16 replicas through solve_groups (fit_groups_kernel); iters = sweeps of every replica, status = the call's
Per case: cost, q (float64), iters, status (int32).

    python tools/dump_knot_bits.py --r10 [OUT.npz]    tests/golden/knot_r10_parent_bits.npz (tests/test_gpu_knot_so_pass.py)

A third fixture, written ONCE with the build of the commit before round 10 (the second-order pass under the segment
floor).  32 fits a case, max_iter = 150, every case on the knot kernel:
  k48, k50, k54, k55, k64   every segment at the floor (no predicated k-step), the bench's K, either side of SEG9, the longest segments
  bankmax, so0              K = 50 in CostBank's max mode (long finishes, rejected trials), and with so_lambda = 0
  resume                    K = 50 in launches of 7 trials: a fit resumed inside the finish enters through the second-order pass
Per case: cost, q (float64), iters, status (int32), evals (float64[1], d2d_fit_solve's stats[3]) and slice (int32[1]): the fits are
rows slice .. slice + 32 of the family's 128, the first such slice on which the evaluation count differs from that of the same
solve with mp_finish = 0 -- a case that never leaves lmder reaches no second-order evaluation and would test nothing."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')) if p not in sys.path]

import numpy as np  # noqa: E402

MAX_ITER = 150
FAMILIES = ('bench', 'k40', 'k64', 'so0', 'bankmax', 'resume')
FIELDS = ('cost', 'q', 'iters', 'status', 'stats')


def scenarios(name):
    """(K, duration, wref, scenarios) of a family"""
    import bench
    from d2dhip import synth
    if name in ('k40', 'k64'):
        K2 = int(name[1:])
        dur = synth.planner_timing(0, (K2 - 1) / 10.0, 10)[2]
        return K2, dur, synth.default_wref(0.1, K2), synth.synth_scenarios(64, seed=5, obj_scale=0.1, K=K2, dist_range=(30. * dur / 4.9, 55. * dur / 4.9))
    dur, wref = bench._plan_consts()
    sc = bench.bench_scenarios(4096)
    if name == 'bankmax':
        return bench.K, dur, wref, synth.variant_scenarios('bankmax', 64, K=bench.K)
    return bench.K, dur, wref, {'bench': sc[:192], 'so0': sc[192:256], 'resume': sc[256:320]}[name]


def run(ctx, name):
    """One family through the knot kernel -> {field: numpy array}"""
    import d2dhip
    K2, dur, wref, sc = scenarios(name)
    dsc = ctx.dev(sc)
    plan = d2dhip.FitPlan(ctx, 6, K2, dur, wref, kernel='knot')
    try:
        assert plan.kernel == 'knot'
        q = plan.init(dsc)
        if name == 'resume':
            plan.begin(len(sc))
            for _ in range(MAX_ITER):
                if plan.iterate(dsc, q, 7, max_iter=MAX_ITER) == 0:
                    break
            cost, iters, status, stats = plan.finish(dsc, q)
        else:
            kw = {'so_lambda': 0.0} if name == 'so0' else {}
            cost, iters, status, stats = plan.solve(dsc, q, max_iter=MAX_ITER, **kw)
        return {'cost': cost.cpu().numpy().astype(np.float64), 'q': q.cpu().numpy().astype(np.float64),
                'iters': iters.cpu().numpy().astype(np.int32), 'status': status.cpu().numpy().astype(np.int32),
                'stats': np.asarray(stats, dtype=np.float64)[1:4].copy()}
    finally:
        plan.close()


R9_B, R9_MAX_ITER = 32, 40
R9_KNOT = ('k23', 'k48', 'k50', 'k55', 'k64', 'so0', 'bankmax')
R9_SHARED = ('fused', 'long', 'groups')
R9_CASES = R9_KNOT + R9_SHARED
R9_FIELDS = ('cost', 'q', 'iters', 'status')
R9_GROUP_AC = 2


def r9_scenarios(name):
    """(K, duration, wref, scenarios [R9_B]) of a case of the round-9 fixture"""
    import bench
    from d2dhip import synth
    if name == 'groups':
        dur, _ = bench._plan_consts()
        s = 1.0 / bench.K
        sc = synth.circle_group_scenarios(R9_GROUP_AC, R9_B // R9_GROUP_AC, dur, bench.K, seed=R9_GROUP_AC, sigma=2.0, obj_scale=1.0)
        return bench.K, dur, (0.02 ** 2, s * 5.0 / 8, s / 8 / synth.G_ACC ** 2), sc.reshape(R9_B, -1)
    if name in ('k50', 'so0', 'bankmax', 'fused'):
        dur, wref = bench._plan_consts()
        sc = synth.variant_scenarios('bankmax', R9_B, K=bench.K) if name == 'bankmax' else bench.bench_scenarios(4096)[:R9_B]
        return bench.K, dur, wref, sc
    K2 = 121 if name == 'long' else int(name[1:])
    dur = synth.planner_timing(0, (K2 - 1) / 10.0, 10)[2]
    return K2, dur, synth.default_wref(0.1, K2), synth.synth_scenarios(R9_B, seed=5, obj_scale=0.1, K=K2, dist_range=(30. * dur / 4.9, 55. * dur / 4.9))


def r9_run(ctx, name):
    """One case of the round-9 fixture -> {field: numpy array}"""
    import d2dhip
    K2, dur, wref, sc = r9_scenarios(name)
    dsc = ctx.dev(sc)
    kernel = {'fused': 'fused', 'long': 'auto', 'groups': 'auto'}.get(name, 'knot')
    plan = d2dhip.FitPlan(ctx, 6, K2, dur, wref, kernel=kernel)
    try:
        assert plan.kernel == {'fused': 'fused', 'long': 'long'}.get(name, 'knot'), (name, plan.kernel)
        q = plan.init(dsc)
        if name == 'groups':
            R = R9_B // R9_GROUP_AC
            cost, sweeps, _ = plan.solve_groups(dsc, q, R9_GROUP_AC, max_sweeps=80, inner_iters=8, tol=1e-12)
            iters, status = plan.group_report(R)[0].astype(np.int32), np.asarray([sweeps], dtype=np.int32)
        else:
            kw = {'so_lambda': 0.0} if name == 'so0' else {}
            cost, iters, status, _ = plan.solve(dsc, q, max_iter=R9_MAX_ITER, **kw)
            iters, status = iters.cpu().numpy().astype(np.int32), status.cpu().numpy().astype(np.int32)
        return {'cost': cost.cpu().numpy().astype(np.float64), 'q': q.cpu().numpy().astype(np.float64), 'iters': iters, 'status': status}
    finally:
        plan.close()


def main_r9(out):
    import d2dhip
    ctx = d2dhip.Context(0)
    arrays = {}
    for name in R9_CASES:
        r = r9_run(ctx, name)
        arrays.update({f'{name}_{k}': v for k, v in r.items()})
        print(name, 'fits', len(r['cost']), 'iters', int(r['iters'].min()), int(r['iters'].max()), 'status', np.bincount(r['status']).tolist(), flush=True)
    ctx.close()
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')


R10_B, R10_POOL = 32, 128
R10_CASES = ('k48', 'k50', 'k54', 'k55', 'k64', 'bankmax', 'so0', 'resume')
R10_FIELDS = ('cost', 'q', 'iters', 'status', 'evals', 'slice')


def r10_scenarios(name, first):
    """(K, duration, wref, scenarios [R10_B]) of a case of the round-10 fixture: rows first .. first + R10_B of its family's R10_POOL"""
    import bench
    from d2dhip import synth
    if name[0] == 'k' and name != 'k50':
        K2 = int(name[1:])
        dur = synth.planner_timing(0, (K2 - 1) / 10.0, 10)[2]
        wref = synth.default_wref(0.1, K2)
        sc = synth.synth_scenarios(R10_POOL, seed=5, obj_scale=0.1, K=K2, dist_range=(30. * dur / 4.9, 55. * dur / 4.9))
    else:
        K2 = bench.K
        dur, wref = bench._plan_consts()
        if name == 'bankmax':
            sc = synth.variant_scenarios('bankmax', R10_POOL, K=K2)
        else:
            base = {'k50': 0, 'so0': 256, 'resume': 512}[name]
            sc = bench.bench_scenarios(4096)[base:base + R10_POOL]
    return K2, dur, wref, sc[first:first + R10_B]


def r10_run(ctx, name, first, **mode_kw):
    """One case of the round-10 fixture -> {field: numpy array}; mode_kw: options of the solve (mp_finish = 0: lmder alone)"""
    import d2dhip
    K2, dur, wref, sc = r10_scenarios(name, first)
    dsc = ctx.dev(sc)
    plan = d2dhip.FitPlan(ctx, 6, K2, dur, wref, kernel='knot')
    try:
        assert plan.kernel == 'knot'
        q = plan.init(dsc)
        kw = dict(mode_kw, so_lambda=0.0) if name == 'so0' else mode_kw
        if name == 'resume':
            plan.begin(len(sc))
            for _ in range(MAX_ITER):
                if plan.iterate(dsc, q, 7, max_iter=MAX_ITER, **kw) == 0:
                    break
            cost, iters, status, stats = plan.finish(dsc, q)
        else:
            cost, iters, status, stats = plan.solve(dsc, q, max_iter=MAX_ITER, **kw)
        return {'cost': cost.cpu().numpy().astype(np.float64), 'q': q.cpu().numpy().astype(np.float64),
                'iters': iters.cpu().numpy().astype(np.int32), 'status': status.cpu().numpy().astype(np.int32),
                'evals': np.asarray(stats, dtype=np.float64)[3:4].copy(), 'slice': np.asarray([first], dtype=np.int32)}
    finally:
        plan.close()


def main_r10(out):
    import d2dhip
    ctx = d2dhip.Context(0)
    arrays = {}
    for name in R10_CASES:
        for first in range(0, R10_POOL, R10_B):
            r, lmder = r10_run(ctx, name, first), r10_run(ctx, name, first, mp_finish=0)
            if r['evals'][0] != lmder['evals'][0]:
                break
        else:
            raise SystemExit(f'{name}: no slice of the family reaches a second-order evaluation')
        arrays.update({f'{name}_{k}': v for k, v in r.items()})
        print(name, 'slice', first, 'iters', int(r['iters'].min()), int(r['iters'].max()), 'status', np.bincount(r['status']).tolist(),
              'evaluations', int(r['evals'][0]), 'with mp_finish = 0', int(lmder['evals'][0]), flush=True)
    ctx.close()
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')


def main():
    import d2dhip
    if len(sys.argv) > 1 and sys.argv[1] == '--r10':
        return main_r10(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'knot_r10_parent_bits.npz'))
    if len(sys.argv) > 1 and sys.argv[1] == '--r9':
        return main_r9(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'knot_r9_parent_bits.npz'))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'knot_parent_bits.npz')
    ctx = d2dhip.Context(0)
    arrays = {}
    for name in FAMILIES:
        r = run(ctx, name)
        arrays.update({f'{name}_{k}': v for k, v in r.items()})
        print(name, 'fits', len(r['cost']), 'iters', int(r['iters'].min()), int(r['iters'].max()), 'status', np.bincount(r['status']).tolist(),
              'evaluations', int(r['stats'][2]), flush=True)
    ctx.close()
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
