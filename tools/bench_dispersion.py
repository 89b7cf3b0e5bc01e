#!/usr/bin/env python3
"""Gust dispersion of tracked plans (include/d2d.h d2d_track_dispersion, ABI 128): what one deterministic pass costs, and what its
margin is worth in a closed loop.  bench.py does not call this.

  bench   65 536 plans x 500 rows through d2d_track_dispersion beside d2d_sim_track_run_gust on the same references (ONE gust flight of
          every plan: the brute-force estimate needs thousands of them per plan), HIP events, alternating, best of --reps.
  demo    plan -> dispersion -> margin -> re-plan -> fly: a perturbed exp_14 (d2dhip.synth.nlp_problems) in a corridor that binds
          (tools/bench_nlp_wind.py's fence leg), the margin of full_sim.dispersion_margin(report, 1.35e-3) at the binding edge, the
          re-plan with GeoFence(margin=), 4096 gust replicas of the re-planned flight, and per row the frequency with which the gust
          share of the deviation exceeds the margin along the edge's normal, next to the target 1.35e-3 -- and the frequency with
          which the aircraft itself crosses the edge, which also contains the gust-free tracking error (reported beside it).
One JSON line each.  A report, not a test.

  python tools/bench_dispersion.py [bench] [demo] [--plans 65536] [--rows 500] [--reps 3] [--replicas 4096] [--sigma 0.3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np   # noqa: E402


def bench(ctx, a):
    import torch
    from d2d.wind import GustModel
    gust = GustModel(1.5, tau=2.0, seed=20241008)
    N, T = a.plans, a.rows + 1
    rng = np.random.default_rng(0)
    t = np.arange(T) * 0.1                                                      # tools/bench_sim_gust.py's tracking references
    ph = rng.uniform(0, 2 * np.pi, N)
    x_ref = 60 * np.sin(0.15 * t[:, None] + ph[None, :]); y_ref = 40 * np.sin(0.3 * t[:, None] + 2 * ph[None, :])
    X0 = np.stack([x_ref[0], y_ref[0], np.arctan2(y_ref[1] - y_ref[0], x_ref[1] - x_ref[0]), np.zeros(N), 12 * np.ones(N)])
    dxr, dyr, dX0 = ctx.dev(x_ref), ctx.dev(y_ref), ctx.dev(X0)
    fns = (lambda o: ctx.track_run(dxr, dyr, dX0, 0.1, record=('X',), out=o, gust=gust),
           lambda o: ctx.track_dispersion(dxr, dyr, gust=gust, dt=0.1),
           lambda o: ctx.track_dispersion(dxr, dyr, gust=gust, dt=0.1, record_P=True))
    outs = [fns[0](None), None, None]
    fns[1](None); ctx.sync()
    best = [1e30] * 3
    for _ in range(a.reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            e0.record(ctx.stream); fn(outs[k]); e1.record(ctx.stream)
            ctx.sync()
            best[k] = min(best[k], e0.elapsed_time(e1) * 1e-3)
    print(json.dumps({'leg': 'bench', 'plans': N, 'rows': a.rows, 'dt': 0.1, 'track_run_gust_s': best[0], 'dispersion_s': best[1],
                      'dispersion_record_P_s': best[2], 'plan_rows_per_s': N * a.rows / best[1], 'flight_drone_steps_per_s': N * a.rows / best[0],
                      'dispersion_over_one_flight': best[1] / best[0],
                      'note': 'the flight is ONE gust replica per plan and records X; the dispersion includes its four derivative launches'}), flush=True)


def demo(ctx, a):
    import d2dhip as Dh
    import full_sim as FS
    import dispersion_ref as DR
    from d2dhip import synth
    from d2d.opty_utils import GeoFence
    from d2d.wind import GustModel
    prob, R = 1.35e-3, a.replicas
    rows, W0, h = synth.nlp_problems(1)
    N = W0.shape[2]
    p0, p1 = rows[0, Dh.SC_X0:Dh.SC_X0 + 2], rows[0, Dh.SC_X1:Dh.SC_X1 + 2]
    d = (p1 - p0) / np.hypot(*(p1 - p0)); ll = float(np.hypot(*(p1 - p0))); nrm = np.array([-d[1], d[0]])
    dsc = ctx.dev(rows)

    def solve(edges):
        W = ctx.dev(np.ascontiguousarray(W0))
        out = ctx.nlp_solve(dsc, W, h) if edges is None else ctx.nlp_solve_fence(dsc, W, h, ctx.dev(edges[None]))
        ctx.sync()
        return W.cpu().numpy()[0], int(out['status'][0].item()), float(out['cost'][0].item())

    Wf, st_f, c_f = solve(None)                                                 # the free plan: where it leaves the leg's axis most
    lat = (Wf[0] - p0[0]) * nrm[0] + (Wf[1] - p0[1]) * nrm[1]
    up = lat.max() >= -lat.min()
    cut = 0.8 * np.abs(lat).max()
    left, right = (cut, ll) if up else (ll, cut)
    verts = [p0 - 0.5 * ll * d - right * nrm, p1 + 0.5 * ll * d - right * nrm, p1 + 0.5 * ll * d + left * nrm, p0 - 0.5 * ll * d + left * nrm]
    fence0 = GeoFence(verts)
    W1, st1, c1 = solve(fence0.lowered())
    gm = GustModel(a.sigma, tau=2.0, seed=7)
    t = np.arange(N) * h
    rep1 = FS.track_dispersion(t, W1[0][:, None], W1[1][:, None], (0., 0.), gm, fence=fence0)
    FS.d2dhip.default_context().sync()
    e = int(np.argmin(rep1['fence_k'].cpu().numpy()[:, 0]))                    # the binding edge: the fewest standard deviations away
    m = FS.dispersion_margin(rep1, prob)
    margin = float(m['fence'][e, 0])
    fence2 = GeoFence(verts, margin=margin)
    W2, st2, c2 = solve(fence2.lowered())
    rep2 = FS.track_dispersion(t, W2[0][:, None], W2[1][:, None], (0., 0.), gm, fence=fence0, record_P=True)
    FS.d2dhip.default_context().sync()
    # fly the re-planned reference: R gust replicas and the gust-free flight, from the state of the first sample the loop uses
    x, y = W2[0], W2[1]
    X0 = DR.reference_states(x, y, h)[1]
    xr, yr = ctx.dev(np.ascontiguousarray(np.tile(x[:, None], (1, R)))), ctx.dev(np.ascontiguousarray(np.tile(y[:, None], (1, R))))
    fl = ctx.track_run(xr, yr, ctx.dev(np.ascontiguousarray(np.tile(X0[:, None], (1, R)))), h, record=('X',), gust=gm, gust_n_ac=1)
    free = ctx.track_run(xr[:, :1].contiguous(), yr[:, :1].contiguous(), ctx.dev(np.ascontiguousarray(X0[:, None])), h, record=('X',))
    ctx.sync()
    ax, ay, b, _ = fence0.lowered()[e]
    Xg, Xf = fl['X'].cpu().numpy(), free['X'].cpu().numpy()
    dev_n = ax * (Xg[:, 0] - Xf[:, 0]) + ay * (Xg[:, 1] - Xf[:, 1])             # the gust share of the deviation along the normal [N][R]
    gap = b - (ax * Xg[:, 0] + ay * Xg[:, 1])                                   # the aircraft's distance to the user's edge
    P = rep2['Ppos'].cpu().numpy()[:, :, 0]
    sn_pred = np.sqrt(ax * ax * P[:, 0] + 2 * ax * ay * P[:, 1] + ay * ay * P[:, 2])
    f_gust = (dev_n > margin).mean(1)
    f_cross = (gap < 0).mean(1)
    ref_gap = b - (ax * x + ay * y)
    i_bind = int(np.argmin(ref_gap[1:])) + 1
    err_free = float(np.abs(ax * (Xf[:, 0, 0] - x) + ay * (Xf[:, 1, 0] - y))[1:].max())
    print(json.dumps({'leg': 'demo', 'nodes': N, 'h': h, 'sigma': a.sigma, 'tau': 2.0, 'replicas': R, 'target_per_row': prob, 'z': m['z'],
                      'status_free_fence_replan': [st_f, st1, st2], 'cost_free_fence_replan': [c_f, c1, c2], 'binding_edge': e,
                      'fence_k_before': float(rep1['fence_k'][e, 0]), 'fence_sn_before': float(rep1['fence_sn'][e, 0]), 'margin': margin,
                      'fence_k_after': float(rep2['fence_k'][e, 0]), 'fence_row_after': int(rep2['fence_row'][e, 0]),
                      'binding_row_of_the_replan': i_bind, 'reference_gap_at_it': float(ref_gap[i_bind]),
                      'sn_predicted_at_it': float(sn_pred[i_bind]), 'sn_sampled_at_it': float(np.sqrt((dev_n[i_bind] ** 2).mean())),
                      'sn_sampled_over_predicted_all_rows_min_max': [float(v) for v in (lambda q: (q.min(), q.max()))(
                          np.sqrt((dev_n[5:] ** 2).mean(1)) / sn_pred[5:])],
                      'gust_share_exceeds_margin_freq_at_it': float(f_gust[i_bind]), 'gust_share_exceeds_margin_freq_max_over_rows': float(f_gust.max()),
                      'expected_at_the_row_of_sig_max': prob, 'crosses_the_edge_freq_at_it': float(f_cross[i_bind]),
                      'crosses_the_edge_freq_max_over_rows': float(f_cross.max()), 'gust_free_error_along_normal_max': err_free,
                      'standard_error_of_a_frequency_at_target': float(np.sqrt(prob * (1 - prob) / R))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('legs', nargs='*', default=['bench', 'demo'])
    ap.add_argument('--plans', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=500)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--sigma', type=float, default=0.3)
    a = ap.parse_args()
    import d2dhip
    ctx = d2dhip.Context(0)
    if 'bench' in a.legs:
        bench(ctx, a)
    if 'demo' in a.legs:
        demo(ctx, a)
    ctx.close()


if __name__ == '__main__':
    main()
