#!/usr/bin/env python3
"""The collocation backend in a wind field at batch scale: B perturbed copies of the reference's exp_14 (121 nodes, hard bounds;
d2dhip.synth.nlp_problems) and one problem alone, in constant wind through d2d_nlp_solve and in a steady (shear) and an unsteady
(gust) field through d2d_nlp_solve_wind.  The fields are tests/wind_ref.py's with the planner's sign (-F: the plan of a plant that flies
F; the shear then blows along the leg, and every problem stays feasible below v_max).  HIP events, best of 3 after a warm-up.
python tools/bench_nlp_wind.py [B ...]     (default 4096 1)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import numpy as np


def main():
    import torch, d2dhip
    from d2dhip import synth
    import wind_ref as WR
    ctx = d2dhip.Context(0)
    fields = {'constant': None, 'steady (shear)': -WR.spline_of(WR.shear), 'unsteady (gust)': -WR.spline_of(WR.gust, t=np.arange(0.0, 14.5, 1.0))}
    for B in [int(x) for x in sys.argv[1:]] or [4096, 1]:
        rows, W0, h = synth.nlp_problems(B)
        dsc = ctx.dev(rows)
        base = None
        for name, F in fields.items():
            times = []
            for rep in range(4):                             # the first launch is the warm-up
                W = ctx.dev(np.ascontiguousarray(W0))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                out = ctx.nlp_solve(dsc, W, h) if F is None else ctx.nlp_solve_wind(dsc, W, h, F)
                e1.record(); torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3)
            best, worst = min(times[1:]), max(times[1:])
            base = base or best
            st = out['status'].cpu().numpy(); it = out['iters'].cpu().numpy()
            print(json.dumps({'B': B, 'wind': name, 'seconds': best, 'spread': worst / best - 1.0, 'problems_per_s': B / best,
                              'vs_constant': best / base, 'converged_frac': float((st == 1).mean()), 'mean_newton_steps': float(it.mean()),
                              'max_newton_steps': int(it.max()), 'max_feas_converged': float(out['feas'].cpu().numpy()[st == 1].max()) if (st == 1).any() else None}),
                  flush=True)


if __name__ == '__main__':
    main()
