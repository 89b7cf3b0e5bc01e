#!/usr/bin/env python3
"""The flight audit at scale: a synthetic history of 65 536 drones (n_ac = 4), 400 rows, audited on the device -- once for the
separation alone (x and y planes), once with two static discs, one moving disc, references and the envelope (x, y, phi, v planes and
the two reference arrays).  Per configuration one JSON line: the median of five windows of ten launches in ms per launch (device events; kernel times alone:
rocprofv3 --kernel-trace --stats -- python tools/bench_audit.py), the bytes the audit
must read (the planes it needs) over that time, and two comparators timed in the same run that are not the code under test: a
device-to-device copy of the same planes (torch.clone; it also writes them) and, for the separation, the row-wise statement in torch
ops that a user can write today.  python tools/bench_audit.py [n_form] [n_rows]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    sys.path.insert(0, _p)
import numpy as np


def median_ms(fn, reps=5, warm=2, calls=10):
    """Median over `reps` event windows of `calls` back-to-back calls each, per call: the queue stays full inside a window unless the
    host enqueues more slowly than the device runs -- the figure is an upper bound of the device time of one call."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return float(np.median(ts))


def main():
    import torch, d2dhip
    n_form = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    n_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    n_ac, dt = 4, 0.5
    N = n_form * n_ac
    ctx = d2dhip.Context(0)
    g = torch.Generator(device=ctx.device); g.manual_seed(1)
    X = torch.empty(n_rows, 5, N, dtype=torch.float64, device=ctx.device)
    X[:, :2] = (torch.rand(1, 2, N, generator=g, device=ctx.device, dtype=torch.float64) * 200 - 100
                + torch.cumsum(torch.rand(n_rows, 2, N, generator=g, device=ctx.device, dtype=torch.float64) * 6 - 3, 0))
    X[:, 2] = 0.0
    X[:, 3] = torch.rand(n_rows, N, generator=g, device=ctx.device, dtype=torch.float64) - 0.5
    X[:, 4] = torch.rand(n_rows, N, generator=g, device=ctx.device, dtype=torch.float64) * 6 + 9
    x_ref = (X[:, 0] + 0.5).contiguous(); y_ref = (X[:, 1] - 0.5).contiguous()
    static = ctx.dev(np.tile(np.array([[[30.0, 20.0, 10.0], [-40.0, 10.0, 15.0]]]), (n_form, 1, 1)))
    knots = ctx.dev(np.tile(np.array([[[[0.0, -80.0, -80.0], [n_rows * dt, 80.0, 80.0]]]]), (n_form, 1, 1, 1)))
    disc = ctx.dev(np.tile(np.array([[[12.0, 0.0]]]), (n_form, 1, 1)))
    plane = n_rows * N * 8

    def torch_rowwise():
        P = X[:, :2].reshape(n_rows, 2, n_form, n_ac)
        D = torch.hypot(P[:, 0, :, :, None] - P[:, 0, :, None, :], P[:, 1, :, :, None] - P[:, 1, :, None, :])
        D = D + torch.eye(n_ac, dtype=torch.float64, device=X.device) * 1e300
        return D.amin(dim=(0, 3))

    configs = [
        ('separation', dict(outputs=('sep',)), 2, lambda: X[:, :2].clone()),
        ('everything', dict(x_ref=x_ref, y_ref=y_ref, static=static, knots=knots, disc=disc, t_start=0.0, d_safe=5.0, err_tol=1.0), 6,
         lambda: (X[:, :2].clone(), X[:, 3:].clone(), x_ref.clone(), y_ref.clone())),
    ]
    for name, kw, planes, copy in configs:
        out = ctx.flight_audit(X, n_ac, dt, **kw)
        torch.cuda.synchronize()
        assert int(out['status'].abs().sum().item()) == 0
        ms = median_ms(lambda: ctx.flight_audit(X, n_ac, dt, **kw))
        ms_copy = median_ms(copy)
        line = {'config': name, 'drones': N, 'n_ac': n_ac, 'rows': n_rows, 'planes': planes, 'bytes': planes * plane, 'audit_ms': ms,
                'audit_TB_per_s': planes * plane / ms * 1e-9, 'copy_ms': ms_copy, 'copy_read_TB_per_s': planes * plane / ms_copy * 1e-9}
        if name == 'separation':
            ms_t = median_ms(torch_rowwise, reps=5, warm=1)
            row = torch_rowwise().reshape(N)
            line.update(torch_rowwise_ms=ms_t, audit_over_torch=ms_t / ms,
                        min_sep_audit=float(out['sep_dist'].min().item()), min_sep_rowwise=float(row.min().item()),
                        drones_closer_between_rows=int((out['sep_dist'] < row - 1e-9).sum().item()))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
