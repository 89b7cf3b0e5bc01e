#!/usr/bin/env python3
"""Cost of flying a wind field (include/d2d.h d2d_wind_field): drone-steps/s of the formation loop at 65 536 drones in constant
wind (the unchanged DPP-quad kernel), in a steady field (a Gaussian vortex) and in an unsteady one (a travelling gust), and of the
tracking loop at bench.py's size, constant wind against a shear field.  One JSON line per run, with the largest fixed-point sweep
count the loop used.

  python tools/bench_sim_wind.py [--drones 65536] [--steps 2000] [--track-steps 500]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np   # noqa: E402


# three smooth fields (gradients <= ~0.2 /s; the same shapes as the fields of tests/test_gpu_wind.py)
def shear(t, x, y):
    return 2.0 + 0.02 * y, 0.5 - 0.01 * x


def vortex(t, x, y, xc=10.0, yc=-40.0, gamma=600.0, rc=60.0):
    dx, dy = x - xc, y - yc
    r2 = np.maximum(dx * dx + dy * dy, 1e-6)
    k = gamma / (2 * np.pi) * (1.0 - np.exp(-r2 / rc ** 2)) / r2
    return -k * dy, k * dx


def gust(t, x, y):
    a = 4.0 * np.exp(-((t - 6.0) / 3.0) ** 2)
    return 1.0 + a * np.exp(-((x - 5.0 * t) / 60.0) ** 2), -0.5 * a * np.sin(y / 50.0)


def spline_of(fn, t=None, h=10.0):
    """The SplineWindField that interpolates fn on a 10 m grid over the formations' box (and the sample times t)."""
    from d2d.wind import SplineWindField
    x = np.arange(-150.0, 150.0 + 0.5 * h, h); y = np.arange(-200.0, 150.0 + 0.5 * h, h)
    if t is None:
        X, Y = np.meshgrid(x, y)
        return SplineWindField.from_samples(x, y, *fn(0.0, X, Y))
    T, Y, X = np.meshgrid(t, y, x, indexing='ij')
    return SplineWindField.from_samples(x, y, *fn(T, X, Y), t=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--drones', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--track-steps', type=int, default=500)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()

    import torch
    import d2dhip
    ctx = d2dhip.Context(0)
    f_vortex = spline_of(vortex)
    f_gust = spline_of(gust, t=np.arange(0.0, 0.1 * max(a.steps, a.track_steps) + 10.0, 0.5))
    f_shear = spline_of(shear)

    def timed(fn):
        out = fn(None); ctx.sync()
        best = 1e30
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            e0.record(ctx.stream); fn(out); e1.record(ctx.stream)
            ctx.sync()
            best = min(best, e0.elapsed_time(e1) * 1e-3)
        return out, best

    n_ac, N = 4, a.drones
    n_form = N // n_ac
    rng = np.random.default_rng(0)
    centres = np.tile(np.array([[0, -20], [25, -20], [25, -100], [0, -100.0]]), (n_form, 1)) + np.repeat(rng.uniform(-5, 5, (n_form, 2)), n_ac, 0)
    X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (N, 1)) + np.concatenate([rng.uniform(-3, 3, (N, 2)), np.zeros((N, 3))], 1)
    dX0, dC, dR = ctx.dev(np.ascontiguousarray(X0.T)), ctx.dev(np.ascontiguousarray(centres.T)), ctx.dev(np.full(N, 60.0))
    rows = a.steps + 1
    for name, wind in (('constant', None), ('steady', f_vortex), ('unsteady', f_gust)):
        kw = {} if wind is None else dict(wind=wind)
        out, sec = timed(lambda o: ctx.gvf_run(dX0, dC, dR, n_ac, rows, 0.05, 15.0, W=(0.7, -0.4), record=(), out=o, **kw))
        rec = {'loop': 'gvf', 'wind': name, 'drones': N, 'steps': a.steps, 'drone_steps_per_s': N * a.steps / sec, 'launch_s': sec,
               'kernel': 'gvf_run_quad_wide_kernel<4>' if wind is None else 'gvf_run_wind_kernel'}
        if wind is not None:
            rec['iter_max'] = int(out['iter_max'].item())
        print(json.dumps(rec), flush=True)
        del out
    del dX0, dC, dR
    torch.cuda.empty_cache()

    T = a.track_steps + 1
    t = np.arange(T) * 0.1
    ph = rng.uniform(0, 2 * np.pi, N)
    x_ref = 60 * np.sin(0.15 * t[:, None] + ph[None, :]); y_ref = 40 * np.sin(0.3 * t[:, None] + 2 * ph[None, :])
    X0t = np.stack([x_ref[0], y_ref[0], np.arctan2(y_ref[1] - y_ref[0], x_ref[1] - x_ref[0]), np.zeros(N), 12 * np.ones(N)])
    dxr, dyr, dX0t = ctx.dev(x_ref), ctx.dev(y_ref), ctx.dev(X0t)
    for name, wind in (('constant', None), ('steady', f_shear)):
        kw = {} if wind is None else dict(wind=wind)
        out, sec = timed(lambda o: ctx.track_run(dxr, dyr, dX0t, 0.1, record=('X', 'U'), out=o, **kw))
        rec = {'loop': 'track', 'wind': name, 'drones': N, 'steps': a.track_steps, 'drone_steps_per_s': N * a.track_steps / sec,
               'launch_s': sec, 'kernel': 'track_run_kernel' if wind is None else 'track_run_wind_kernel'}
        if wind is not None:
            rec['iter_max'] = int(out['iter_max'].item())
        print(json.dumps(rec), flush=True)
        del out
    ctx.close()


if __name__ == '__main__':
    main()
