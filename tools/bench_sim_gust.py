#!/usr/bin/env python3
"""Cost of flying stochastic gusts (include/d2d.h d2d_gust): drone-steps/s of each gust loop against its twin, timed in ONE process,
alternating twin / gust, best of --reps, at tools/bench_sim_wind.py's sizes: 65 536 drones x 2000 formation steps (constant wind and a
steady vortex, formations of four; constant wind in formations of three, where the twin is the general kernel too) and x 500 tracking
steps (constant wind and a shear).  The twin is untouched by the gust code: it is the yardstick.  One JSON line per pair.

  python tools/bench_sim_gust.py [--drones 65536] [--steps 2000] [--track-steps 500] [--reps 3] [--form-corr 0.36]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tools')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np   # noqa: E402

from bench_sim_wind import shear, spline_of, vortex   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--drones', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--track-steps', type=int, default=500)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--form-corr', type=float, default=0.36)
    a = ap.parse_args()

    import torch
    import d2dhip
    from d2d.wind import GustModel
    ctx = d2dhip.Context(0)
    gust = GustModel(1.5, tau=2.0, seed=20241008, form_corr=a.form_corr)
    f_vortex, f_shear = spline_of(vortex), spline_of(shear)

    def pair(twin, gusty):
        """best-of-reps seconds of the two launches, alternating (a warm-up of each first: its buffers are reused)"""
        outs = [twin(None), gusty(None)]
        ctx.sync()
        best = [1e30, 1e30]
        for _ in range(a.reps):
            for k, fn in enumerate((twin, gusty)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.sync()
                e0.record(ctx.stream); fn(outs[k]); e1.record(ctx.stream)
                ctx.sync()
                best[k] = min(best[k], e0.elapsed_time(e1) * 1e-3)
        return best

    def report(loop, wind, N, steps, kernels, best, **more):
        rec = {'loop': loop, 'wind': wind, 'drones': N, 'steps': steps, 'twin_kernel': kernels[0], 'gust_kernel': kernels[1],
               'twin_drone_steps_per_s': N * steps / best[0], 'gust_drone_steps_per_s': N * steps / best[1], 'ratio': best[0] / best[1],
               'twin_s': best[0], 'gust_s': best[1], 'form_corr': a.form_corr, **more}
        print(json.dumps(rec), flush=True)

    rng = np.random.default_rng(0)
    rows = a.steps + 1
    for n_ac, cases in ((4, (('constant', None, ('gvf_run_quad_wide_kernel<4>', 'gvf_run_gust_kernel')),
                             ('steady', f_vortex, ('gvf_run_wind_kernel', 'gvf_run_wind_gust_kernel')))),
                        (3, (('constant', None, ('gvf_run_kernel', 'gvf_run_gust_kernel')),))):
        n_form = a.drones // n_ac
        N = n_form * n_ac
        c4 = np.array([[0, -20], [25, -20], [25, -100], [0, -100.0]])[:n_ac]
        centres = np.tile(c4, (n_form, 1)) + np.repeat(rng.uniform(-5, 5, (n_form, 2)), n_ac, 0)
        X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (N, 1)) + np.concatenate([rng.uniform(-3, 3, (N, 2)), np.zeros((N, 3))], 1)
        dX0, dC, dR = ctx.dev(np.ascontiguousarray(X0.T)), ctx.dev(np.ascontiguousarray(centres.T)), ctx.dev(np.full(N, 60.0))
        for name, wind, kernels in cases:
            kw = {} if wind is None else dict(wind=wind)
            best = pair(lambda o: ctx.gvf_run(dX0, dC, dR, n_ac, rows, 0.05, 15.0, W=(0.7, -0.4), record=(), out=o, **kw),
                        lambda o: ctx.gvf_run(dX0, dC, dR, n_ac, rows, 0.05, 15.0, W=(0.7, -0.4), record=(), out=o, gust=gust, **kw))
            report('gvf', name, N, a.steps, kernels, best, n_ac=n_ac)
        del dX0, dC, dR
        torch.cuda.empty_cache()

    N = a.drones
    T = a.track_steps + 1
    t = np.arange(T) * 0.1
    ph = rng.uniform(0, 2 * np.pi, N)
    x_ref = 60 * np.sin(0.15 * t[:, None] + ph[None, :]); y_ref = 40 * np.sin(0.3 * t[:, None] + 2 * ph[None, :])
    X0t = np.stack([x_ref[0], y_ref[0], np.arctan2(y_ref[1] - y_ref[0], x_ref[1] - x_ref[0]), np.zeros(N), 12 * np.ones(N)])
    dxr, dyr, dX0t = ctx.dev(x_ref), ctx.dev(y_ref), ctx.dev(X0t)
    for name, wind, kernels in (('constant', None, ('track_run_kernel', 'track_run_gust_kernel')),
                                ('steady', f_shear, ('track_run_wind_kernel', 'track_run_wind_gust_kernel'))):
        kw = {} if wind is None else dict(wind=wind)
        best = pair(lambda o: ctx.track_run(dxr, dyr, dX0t, 0.1, record=('X', 'U'), out=o, **kw),
                    lambda o: ctx.track_run(dxr, dyr, dX0t, 0.1, record=('X', 'U'), out=o, gust=gust, gust_n_ac=4, **kw))
        report('track', name, N, a.track_steps, kernels, best)
    ctx.close()


if __name__ == '__main__':
    main()
