#!/usr/bin/env python3
"""The fleet audit at scale: formations of four spread over a square at a fixed density (about four aircraft per 3 x 3 grid cells),
256 rows, audited across formations on the device (Context.fleet_audit).  One JSON line per drone count: the median of five windows
of launches in ms per audit (device events), drone-rows per second, the measured mean number of aircraft in the nine cells a query
looks into (own formation included: what a list walk meets, slot sharing aside), and, as the cost of reading the same history, the
time of flight_audit(outputs=('sep',)) on it.  At 8192 drones and a few rows one more line: the row-wise all-pairs minimum with
torch.cdist, which is what a user can write today (it sees no approach between rows).  The last line is the measured condition:
time(65 536) / time(32 768) < 3 at equal density (linear work: 2, all pairs: 4).
python tools/bench_fleet_audit.py [n_rows]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    sys.path.insert(0, _p)
import numpy as np

N_AC, DT, D_LOOK, STEP_MAX, D_SAFE = 4, 0.5, 10.0, 3.0, 5.0
EDGE = (D_LOOK + 2 * STEP_MAX) * (1 + 2.0 ** -16)
PER_9_CELLS = 4.0                      # aircraft per 3 x 3 cells


def median_ms(fn, reps=5, warm=2, calls=4):
    """Median over `reps` event windows of `calls` back-to-back calls each, per call."""
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


def history(ctx, N, n_rows, seed=1):
    """Formations of N_AC within 15 m of a centre drawn uniformly in a square of N * 9 EDGE^2 / PER_9_CELLS m^2; every aircraft walks
    up to 2 m per row and axis (a step <= 2.83 m < STEP_MAX)."""
    import torch
    g = torch.Generator(device=ctx.device); g.manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=ctx.device, dtype=torch.float64)     # noqa: E731
    side = float(np.sqrt(N * 9.0 * EDGE * EDGE / PER_9_CELLS))
    centre = (rnd(1, 2, N // N_AC) * side - side / 2).repeat_interleave(N_AC, dim=2)
    X = torch.zeros(n_rows, 5, N, dtype=torch.float64, device=ctx.device)
    X[:, :2] = centre + rnd(1, 2, N) * 30 - 15 + torch.cumsum(rnd(n_rows, 2, N) * 4 - 2, 0)
    X[:, 4] = 12.0
    return X, side


def in_nine_cells(X, rows=(0, -1)):
    """Mean number of aircraft (itself and its formation included) in the 3 x 3 cells around an aircraft, over the given rows."""
    import torch
    tot = 0.0
    for r in rows:
        c = torch.floor(X[r, :2] / EDGE).to(torch.int64)
        c = c - c.min(dim=1, keepdim=True).values + 1
        M = int(c.max().item()) + 2
        keys, counts = torch.unique(c[0] * M + c[1], return_counts=True)
        n = torch.zeros(c.shape[1], dtype=torch.int64, device=X.device)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                k = (c[0] + dx) * M + (c[1] + dy)
                i = torch.searchsorted(keys, k).clamp(max=len(keys) - 1)
                n += torch.where(keys[i] == k, counts[i], torch.zeros_like(counts[i]))
        tot += float(n.double().mean().item())
    return tot / len(rows)


def main():
    import torch, d2dhip
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    ctx = d2dhip.Context(0)
    ms_of = {}
    for N in (32768, 65536):
        X, side = history(ctx, N, n_rows)
        kw = dict(d_safe=D_SAFE)
        out = ctx.fleet_audit(X, N_AC, DT, D_LOOK, STEP_MAX, **kw)
        torch.cuda.synchronize()
        assert int(out['status'].abs().sum().item()) == 0
        ms = median_ms(lambda: ctx.fleet_audit(X, N_AC, DT, D_LOOK, STEP_MAX, **kw))
        ms_in = median_ms(lambda: ctx.flight_audit(X, N_AC, DT, outputs=('sep',)), calls=10)
        ms_of[N] = ms
        seen = out['near_partner'] >= 0
        print(json.dumps({'config': 'fleet', 'drones': N, 'n_ac': N_AC, 'rows': n_rows, 'side_m': side, 'd_look': D_LOOK, 'step_max': STEP_MAX,
                          'in_nine_cells': in_nine_cells(X), 'fleet_ms': ms, 'drone_rows_per_s': N * n_rows / ms * 1e3,
                          'flight_audit_sep_ms': ms_in, 'fleet_over_reading': ms / ms_in, 'drones_that_see_someone': int(seen.sum().item()),
                          'min_near_dist': float(out['near_dist'][seen].min().item()), 'rows_closer_than_d_safe': int(out['near_count'].sum().item())}),
              flush=True)
        del X, out
    # what a user can write today: all pairs, row by row
    N, rows = 8192, 8
    X, _ = history(ctx, N, rows)
    own = (torch.arange(N, device=ctx.device)[:, None] // N_AC) == (torch.arange(N, device=ctx.device)[None, :] // N_AC)

    def cdist_rowwise():
        best = torch.full((N,), float('inf'), dtype=torch.float64, device=ctx.device)
        for r in range(rows):
            P = X[r, :2].t().contiguous()
            best = torch.minimum(best, torch.cdist(P, P).masked_fill(own, float('inf')).amin(dim=1))
        return best

    ms_c = median_ms(cdist_rowwise, reps=3, warm=1, calls=1)
    ms_f = median_ms(lambda: ctx.fleet_audit(X, N_AC, DT, D_LOOK, STEP_MAX))
    out = ctx.fleet_audit(X, N_AC, DT, D_LOOK, STEP_MAX)
    row = cdist_rowwise()
    seen = out['near_partner'] >= 0
    print(json.dumps({'config': 'cdist', 'drones': N, 'rows': rows, 'cdist_rowwise_ms': ms_c, 'fleet_ms': ms_f, 'cdist_over_fleet': ms_c / ms_f,
                      'never_farther_than_rowwise': bool((out['near_dist'][seen] <= row[seen] + 1e-9).all().item()),
                      'drones_closer_between_rows': int((out['near_dist'][seen] < row[seen] - 1e-9).sum().item())}), flush=True)
    ratio = ms_of[65536] / ms_of[32768]
    print(json.dumps({'config': 'scaling', 'ms_32768': ms_of[32768], 'ms_65536': ms_of[65536], 'ratio': ratio, 'bound': 3.0, 'ok': ratio < 3.0}),
          flush=True)
    return 0 if ratio < 3.0 else 1


if __name__ == '__main__':
    sys.exit(main())
