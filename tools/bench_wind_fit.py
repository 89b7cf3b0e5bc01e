#!/usr/bin/env python3
"""d2d_wind_fit at fleet size: samples/s and ms per fit for N drones x n_rows rows of history on a steady and an unsteady grid.
The history is synthesised on the device (formations of four on circles of 60 m at 15 m/s in a shear plus a head wind that grows
with time: what phase 1 of the mission flies, without simulating it), so the drones of a formation share spline cells and a drone
stays in one for tens of rows, as in a flown history.  One HIP event pair around `reps` whole calls (all five kernels) after a warm-up; the
wavefront count of the accumulation launch is varied to show what the launch geometry costs: the results do not depend on it.
python tools/bench_wind_fit.py [N_drones [n_rows [reps]]]     (default 65536 2700 5)
Prints one JSON line per case."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    sys.path.insert(0, _p)
import numpy as np


def history(ctx, N, n_rows, dt, n_ac=4, seed=1):
    """dev [n_rows][5][N]: circles of 60 m flown at 15 m/s airspeed, drifting with the wind (2 + 0.02 y + 0.005 t, 0.5 - 0.01 x)."""
    import torch
    g = torch.Generator(device=ctx.device); g.manual_seed(seed)
    n_form = N // n_ac
    cx = (torch.rand(n_form, generator=g, device=ctx.device, dtype=torch.float64) * 100.0 - 50.0).repeat_interleave(n_ac)
    cy = (torch.rand(n_form, generator=g, device=ctx.device, dtype=torch.float64) * 100.0 - 50.0).repeat_interleave(n_ac)
    ph = torch.rand(N, generator=g, device=ctx.device, dtype=torch.float64) * 6.283185307179586
    X = torch.empty(n_rows, 5, N, dtype=torch.float64, device=ctx.device)
    x, y = cx + 60.0 * torch.cos(ph), cy + 60.0 * torch.sin(ph)
    for i in range(n_rows):
        t = i * dt
        psi = ph + 0.25 * t + 1.5707963267948966
        X[i, 0], X[i, 1], X[i, 2], X[i, 3], X[i, 4] = x, y, psi, 0.36, 15.0
        # midpoint rule for the next row: the fit's own trapezoid error is then what a flown history shows
        psm = psi + 0.125 * dt
        x = x + dt * (15.0 * torch.cos(psm) + 0.02 * (y - cy) + 0.005 * t)      # (relative shear: the formations stay on their circles' scale)
        y = y + dt * (15.0 * torch.sin(psm) - 0.01 * (x - cx))
    return X


def main():
    import torch
    import d2dhip
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    n_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 2700
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dt = 0.05
    ctx = d2dhip.Context(0)
    X = history(ctx, N, n_rows, dt)
    ctx.sync()
    T = n_rows * dt
    grids = {'steady 12x12': d2dhip.WindFieldC(1, 12, 12, 0, 0.0, 1.0, -300.0, 60.0, -300.0, 60.0, None),
             'unsteady 8x12x12': d2dhip.WindFieldC(8, 12, 12, 0, -1.0, (T + 2.0) / 5.0, -300.0, 60.0, -300.0, 60.0, None)}
    samples = (n_rows - 1) * N
    for name, g in grids.items():
        for waves in (0, 2048, 32768):
            kw = dict(w_max=50.0, lam=1e-2, mu=1e-6, cg_tol=1e-10, cg_max=2000, waves=waves)
            out = ctx.wind_fit(X, 4, dt, g, **kw)
            ctx.sync()
            st = out['stats'].cpu().numpy()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ctx.wind_fit(X, 4, dt, g, **kw)
            e1.record()
            ctx.sync()
            ms = e0.elapsed_time(e1) / reps
            print(json.dumps(dict(case=name, drones=N, n_rows=n_rows, waves=waves or 'library', samples=samples, used=int(st[0]), ms_per_fit=round(ms, 3),
                                  msamples_per_s=round(samples / ms / 1e3, 1), cg_iters=int(st[6]))), flush=True)


if __name__ == '__main__':
    main()
