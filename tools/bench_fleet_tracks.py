#!/usr/bin/env python3
"""fleet_tracks next to fleet_audit on the SAME history in the same job, at the density of tools/bench_fleet_audit.py (formations of
four, about four aircraft per 3 x 3 grid cells): 65 536 drones x 256 rows and 8192 x 8.  One JSON line per shape and n_mov: the median
of five windows of launches in ms per call (device events) for both calls, their ratio, and what the lists held (formations with
partners, with more partners than slots).  Then one deconflict_plans run over worlds of four formations of one aircraft whose legs
cross in the middle of the world (41 nodes): the time of every round (host clock around a synchronised round: the loop reads one
scalar per round) and what the final audit says -- once with the discs a soft cost (margin 4 m) and once with hard=True at margin 0
(d2d_nlp_solve_keepout_moving: the separation is then held, not reached), both from the same independent plans.
python tools/bench_fleet_tracks.py [n_rows] [worlds] [deconflict]     (a third argument: the deconflict runs only)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, _p)
import numpy as np

from bench_fleet_audit import N_AC, DT, D_LOOK, STEP_MAX, D_SAFE, history, median_ms


def tracks_vs_audit(ctx, N, n_rows):
    import torch
    X, _ = history(ctx, N, n_rows)
    ms_a = median_ms(lambda: ctx.fleet_audit(X, N_AC, DT, D_LOOK, STEP_MAX, d_safe=D_SAFE))
    for n_mov in (1, 4, 8):
        n_knot = min(32, n_rows)
        fn = lambda: ctx.fleet_tracks(X, N_AC, DT, D_LOOK, STEP_MAX, D_SAFE, n_mov=n_mov, n_knot=n_knot)     # noqa: E731
        out = fn()
        torch.cuda.synchronize()
        assert int(out['status'].abs().sum().item()) == 0
        ms_t = median_ms(fn)
        nc = out['n_conf']
        print(json.dumps({'config': 'tracks', 'drones': N, 'n_ac': N_AC, 'rows': n_rows, 'n_mov': n_mov, 'n_knot': n_knot, 'fleet_audit_ms': ms_a,
                          'fleet_tracks_ms': ms_t, 'tracks_over_audit': ms_t / ms_a, 'formations_with_partners': int((nc > 0).sum().item()),
                          'more_partners_than_slots': int((nc == n_mov + 1).sum().item()),
                          'max_chord_err_m': float(out['chord_err'].max().item())}), flush=True)
        del out


def deconflict_run(ctx, worlds):
    """Worlds of four single aircraft on 48 m legs: formations 0 and 1 cross at right angles and are both at the crossing at node 20,
    formations 2 and 3 do the same 200 m to the east (scenario 1 of tests/test_gpu_deconflict.py, twice per world); the worlds are
    replicas that lie on top of each other and only their world ids keep them apart.  Priority: the formation index.  round_ms: from one fleet_tracks call to the next; the last entry is the closing
    fleet_tracks call, which finds nothing left to do, and the final audit."""
    import torch, d2dhip, full_sim
    N, h, R = 41, 0.1, 4 * worlds
    rows = np.zeros((R, d2dhip.SCEN_STRIDE))
    th = np.tile([0.0, np.pi / 2, 0.0, np.pi / 2], worlds)
    c = np.tile([0.0, 0.0, 200.0, 200.0], worlds)
    rows[:, d2dhip.SC_X0], rows[:, d2dhip.SC_Y0], rows[:, d2dhip.SC_PSI0] = c - 24 * np.cos(th), -24 * np.sin(th), th
    rows[:, d2dhip.SC_X1], rows[:, d2dhip.SC_Y1], rows[:, d2dhip.SC_PSI1] = c + 24 * np.cos(th), 24 * np.sin(th), th
    rows[:, d2dhip.SC_VSP], rows[:, d2dhip.SC_KV], rows[:, d2dhip.SC_KPHI], rows[:, d2dhip.SC_S], rows[:, d2dhip.SC_KOBS] = 12.0, 70.0, 1.0, 1.0 / N, 100.0
    rows[:, d2dhip.SC_PHIMAX], rows[:, d2dhip.SC_VMIN], rows[:, d2dhip.SC_VMAX] = np.deg2rad(30.0), 9.0, 14.0
    W0 = np.zeros((R, 5, N))
    s = np.linspace(0.0, 1.0, N)
    W0[:, 0] = rows[:, d2dhip.SC_X0, None] + s * (rows[:, d2dhip.SC_X1] - rows[:, d2dhip.SC_X0])[:, None]
    W0[:, 1] = rows[:, d2dhip.SC_Y0, None] + s * (rows[:, d2dhip.SC_Y1] - rows[:, d2dhip.SC_Y0])[:, None]
    W0[:, 2], W0[:, 4] = th[:, None], 12.0
    scen, W = ctx.dev(rows), ctx.dev(W0)
    world = np.repeat(np.arange(worlds), 4)
    full_sim.deconflict_plans(ctx, scen[:4].contiguous(), ctx.dev(W0[:4]), h, 1, d_sep=4.0, margin=4.0, d_look=10.0, step_max=2.0)      # warm-up: one world
    full_sim.deconflict_plans(ctx, scen[:4].contiguous(), ctx.dev(W0[:4]), h, 1, d_sep=4.0, margin=0.0, d_look=10.0, step_max=2.0, hard=True)
    t = time.perf_counter()
    ctx.nlp_solve(scen, W, h)
    torch.cuda.synchronize()
    t_plan = time.perf_counter() - t
    tracks = ctx.fleet_tracks
    W_indep = W.clone()
    for label, kw in (('soft', dict(margin=4.0)), ('hard', dict(margin=0.0, hard=True))):
        _deconflict_timed(ctx, tracks, label, kw, scen, W_indep.clone(), h, world, worlds, R, N, t_plan)


def _deconflict_timed(ctx, tracks, label, kw, scen, W, h, world, worlds, R, N, t_plan):
    import torch, full_sim
    stamps = []

    def timed_tracks(*a, **kw):                      # a round begins with its fleet_tracks call
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return tracks(*a, **kw)

    ctx.fleet_tracks = timed_tracks
    try:
        _, info = full_sim.deconflict_plans(ctx, scen, W, h, 1, world=world, d_sep=4.0, d_look=10.0, step_max=2.0, max_rounds=6, **kw)
    finally:
        del ctx.fleet_tracks
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    near = info['audit']['near_dist']
    st = torch.cat([sv['status'] for sv in info['solves']]).cpu().numpy() if info['solves'] else np.zeros(0, int)
    print(json.dumps({'config': 'deconflict', 'discs': label, 'margin': kw['margin'], 'worlds': worlds, 'formations': R, 'n_ac': 1, 'nodes': N, 'independent_plan_ms': t_plan * 1e3,
                      'rounds': info['rounds'], 'replanned': info['replanned'], 'round_ms': [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])],
                      'truncated': info['truncated'], 'not_converged': len(info['not_converged']), 'refused': len(info['refused']),
                      'unresolved': len(info['unresolved']), 'status_counts': {int(k): int((st == k).sum()) for k in np.unique(st)},
                      'min_near_dist': float(near[torch.isfinite(near)].min().item())}), flush=True)


def main():
    import d2dhip
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    worlds = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    ctx = d2dhip.Context(0)
    if len(sys.argv) <= 3:
        tracks_vs_audit(ctx, 65536, n_rows)
        tracks_vs_audit(ctx, 8192, 8)
    deconflict_run(ctx, worlds)
    return 0


if __name__ == '__main__':
    sys.exit(main())
